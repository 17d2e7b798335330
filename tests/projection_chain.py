"""The projection operator's whole chain on the CPU, forward and hand-chained VJP, for the row form, the packed form and the array
form of the projection (TEST INFRASTRUCTURE: numpy + CPU torch, nothing here touches the GPU or imports the package).

    [quantizer grid -> exp / sigmoid -> temporal slice]  ->  projection  ->  per-view opacities  ->  per-view colours (or SH)

Every floating-point piece already lives in ``oracle/``: ``gs_oracle.projection_fwd / projection_bwd / sh_fwd / sh_bwd`` (C, built once
in float32 and once in float64 from the same source), ``unfused_oracle.temporal_slice`` (torch) and ``gs_oracle.quant_round_fwd``.
``chain(bits, ...)`` strings them together in ``bits`` = 64 (the ground truth) or 32 (the reference's own arithmetic: the yardstick for
how far ANY float32 evaluation is from the truth) from the same float32 inputs; what is hand-written here -- the opacity / compensation
product rule, the per-camera sums, the clamp gate of the SH colours, the view-direction gradient added to ``v_means`` (and, with
``need_viewmats``, carried through the camera centre ``inverse(viewmats)[:, :3, 3]`` into ``v_viewmats``), the activations and the
straight-through quantizer in front of the slice -- is held against central differences by tests/test_projection_chain_cpu.py.

One deliberate deviation from the reference's autograd: ``torch.inverse``'s backward, ``-inv^T G inv^T``, also puts a gradient on the bottom
row of ``viewmats`` (the camera centre times the centre's cotangent).  That row is the constant (0, 0, 0, 1) of a world-to-camera matrix; the
chain takes rows 0..2 of the same expression and leaves the bottom row of ``v_viewmats`` zero, as ``O.projection_bwd`` and the kernels do."""
from __future__ import annotations

import numpy as np
import torch

from oracle import gs_oracle as O
from oracle import unfused_oracle as UO

GATE_EPS = 1e-4  # an SH colour this close to the clamp at zero may fall on either side of it in another evaluation
DYN_KEYS = ("motion", "omega", "trbf_center", "trbf_scale")


def _np(bits):
    return np.float64 if bits == 64 else np.float32


def _grid(x, bounds):
    """The round-to-grid quantizer's values (float32, as the kernels and ``STE`` compute them) of the float32 array ``x``."""
    lo, hi, nbits = bounds
    return O.quant_round_fwd(np.asarray(x, np.float32), lo, hi, nbits)[1]


def _slice(bits, P, dyn):
    """-> (leaves, sliced): torch leaves (requires_grad) of every parameter in ``P`` and the tensors the projection sees."""
    dt = torch.float64 if bits == 64 else torch.float32
    leaves = {k: torch.tensor(np.asarray(v, _np(bits)), dtype=dt, requires_grad=True) for k, v in P.items() if not k.startswith("_")}
    s = dict(leaves)
    if dyn is None:
        return leaves, s
    raw, quant = tuple(dyn.get("raw", ())), dict(dyn.get("quantize") or {})
    for k, bounds in quant.items():
        # straight-through: the grid value (float32 arithmetic on the float32 parameter, upcast) with the identity gradient
        q = torch.tensor(np.asarray(_grid(P[k], bounds), _np(bits)), dtype=dt)
        s[k] = leaves[k] + (q - leaves[k]).detach()
    if "scales" in raw:
        s["scales"] = torch.exp(s["scales"])
    if "opacities" in raw:
        s["opacities"] = torch.sigmoid(s["opacities"])
    tscale = torch.exp(s["trbf_scale"]) if "trbf_scale" in raw else s["trbf_scale"]
    t = float(dyn["t"])
    m_t, q_t, o_t, trbf = UO.temporal_slice(s["means"], s["motion"], s["quats"], s["omega"], s["opacities"], s["trbf_center"], tscale, t)
    if "_motion_center" in P:
        # (for finite differences only: the slice DETACHES t - trbf_center where it moves the splat, so a difference quotient in
        # trbf_center must hold that use of it still; the temporal basis above takes the perturbed centre)
        held = torch.tensor(np.asarray(P["_motion_center"], _np(bits)), dtype=dt)
        m_t, q_t, _, _ = UO.temporal_slice(s["means"], s["motion"], s["quats"], s["omega"], s["opacities"], held, tscale, t)
    s["means"], s["quats"], s["opacities"], s["trbf"] = m_t, q_t, o_t, trbf
    return leaves, s


def chain(bits, P, viewmats, Ks, width, height, camera_model="pinhole", antialiased=False, sh_degree=None, dynamic=None,
          packed_formula=False, need_viewmats=False, cot=None, vis=None, eps2d=0.3, near_plane=0.01, far_plane=1e10, radius_clip=0.0):
    """Forward and, with ``cot``, the VJP of one projection call in ``bits``-bit arithmetic.

    P         float arrays by name: ``means``, ``covars`` [N,6] or ``quats`` + ``scales``, optionally ``opacities`` [N] (row form; without
              them the array / packed form, whose fifth output is the compensation itself), ``colors`` [N,3] or ``sh`` [N,K,3] (with
              ``sh_degree``), and with ``dynamic`` the four temporal tensors ``motion, omega, trbf_center, trbf_scale``.
    dynamic   ``dict(t=..., raw=(names), quantize={name: (lo, hi, bits)}, min_trbf=None)``, as ``DynamicSlice`` takes them.
    cot       cotangents [C,N,...] by output name among ``means2d, depths, conics, opacities, colors, compensations`` (missing: zero).
    vis       bool [C,N]: the pairs the VJP runs over (default: this evaluation's own ``radii > 0``).
    -> (out, grads): ``out`` holds radii, means2d, depths, conics, [compensations], [opacities], [colors], [sh_raw: the SH value before + 0.5 and the clamp], ``gate`` (bool, like
    colours: entries whose SH value lies within GATE_EPS of the clamp); ``grads`` (None without ``cot``) one array per entry of ``P`` plus
    ``viewmats`` [C,4,4] with ``need_viewmats``."""
    f = _np(bits)
    leaves, s = _slice(bits, P, dynamic)
    n = lambda t: np.ascontiguousarray(t.detach().numpy(), f)  # noqa: E731
    means = n(s["means"])
    covars = n(s["covars"]) if "covars" in s else None
    quats, scales = (None, None) if covars is not None else (n(s["quats"]), n(s["scales"]))
    vm, K = np.asarray(viewmats, f), np.asarray(Ks, f)
    C, N = vm.shape[0], means.shape[0]
    rows = "opacities" in s
    with O.precision(bits):
        radii, means2d, depths, conics, comp = O.projection_fwd(
            means, covars, quats, scales, vm, K, width, height, eps2d, near_plane, far_plane, radius_clip,
            calc_compensations=antialiased, camera_model=camera_model, packed_formula=packed_formula)
        if dynamic is not None and dynamic.get("min_trbf") is not None:
            off = n(s["trbf"]) <= f(dynamic["min_trbf"])  # culled by the projection: no radius, no outputs, no gradient
            radii[:, off] = 0
            for a in (means2d, depths, conics, comp):
                if a is not None:
                    a[:, off] = 0
        seen = radii > 0
        out = dict(radii=radii, means2d=means2d, depths=depths, conics=conics)
        if comp is not None:
            out["compensations"] = comp
        if rows:
            opacity = n(s["opacities"])
            out["opacities"] = (opacity[None] * comp if antialiased else np.broadcast_to(opacity[None], (C, N)) * seen).astype(f)
        gate = np.zeros((C, N, 3), bool)
        dirs = sh_raw = coeffs = None
        if "sh" in s:
            campos = np.linalg.inv(np.asarray(viewmats, np.float64))[:, :3, 3].astype(f)
            dirs = np.ascontiguousarray(means[None] - campos[:, None])
            coeffs = np.ascontiguousarray(np.broadcast_to(n(s["sh"])[None], (C,) + tuple(s["sh"].shape)))
            sh_raw = O.sh_fwd(sh_degree, dirs, coeffs, masks=seen)
            out["colors"] = (np.maximum(sh_raw + f(0.5), 0) * seen[..., None]).astype(f)
            gate = (np.abs(sh_raw + f(0.5)) <= GATE_EPS) & seen[..., None]
            out["sh_raw"] = sh_raw
        elif "colors" in s:
            out["colors"] = (np.broadcast_to(n(s["colors"])[None], (C, N, 3)) * seen[..., None]).astype(f)
        out["gate"] = gate
        if cot is None:
            return out, None

        vis = seen if vis is None else np.asarray(vis, bool)
        z = lambda key, shape: np.ascontiguousarray(np.asarray(cot.get(key, np.zeros(shape)), f) * vis.reshape(vis.shape + (1,) * (len(shape) - 2)))  # noqa: E731
        v_m2, v_d, v_cn = z("means2d", (C, N, 2)), z("depths", (C, N)), z("conics", (C, N, 3))
        v_sliced = {}
        if rows:
            v_oc = z("opacities", (C, N))
            v_sliced["opacities"] = (v_oc * comp).sum(0) if antialiased else v_oc.sum(0)
            v_comp = np.ascontiguousarray(v_oc * opacity[None]) if antialiased else None
        else:
            v_comp = z("compensations", (C, N)) if antialiased else None
        v_means, v_covars, v_quats, v_scales, v_view = O.projection_bwd(
            means, covars, quats, scales, vm, K, width, height, eps2d, camera_model, vis.astype(np.int32), conics, comp, v_m2, v_d, v_cn,
            v_comp, need_viewmats=need_viewmats)
        if "sh" in s:
            v_col = z("colors", (C, N, 3)) * (sh_raw + f(0.5) > 0)  # the clamp's gate
            v_coeffs, v_dirs = O.sh_bwd(sh_degree, dirs, coeffs, np.ascontiguousarray(v_col), masks=vis)
            v_sliced["sh"] = v_coeffs.sum(0)
            v_means = v_means + v_dirs.sum(0)  # dirs = means - campos
            if need_viewmats:
                # campos = inverse(viewmats)[:, :3, 3] and d inverse = -inverse dV inverse (float64, as the inverse itself), rows 0..2:
                # the bottom row of a world-to-camera matrix is the constant (0, 0, 0, 1)
                inv = np.linalg.inv(np.asarray(viewmats, np.float64))
                v_campos = -v_dirs.sum(1).astype(np.float64)
                v_view = v_view.copy()
                v_view[:, :3] += (-np.einsum("cai,ca,cj->cij", inv[:, :3, :3], v_campos, inv[:, :, 3])).astype(f)
        elif "colors" in s:
            v_sliced["colors"] = z("colors", (C, N, 3)).sum(0)
    v_sliced["means"] = v_means
    if covars is not None:
        v_sliced["covars"] = v_covars
    else:
        v_sliced["quats"], v_sliced["scales"] = v_quats, v_scales
    # back through the slice, the activations and the straight-through quantizer
    keys = [k for k in v_sliced if s[k].requires_grad]
    dt = next(iter(leaves.values())).dtype
    torch.autograd.backward([s[k] for k in keys], [torch.tensor(np.asarray(v_sliced[k], f), dtype=dt).reshape(s[k].shape) for k in keys])
    grads = {k: (np.zeros(t.shape, f) if t.grad is None else t.grad.numpy().astype(f)) for k, t in leaves.items()}
    if need_viewmats:
        grads["viewmats"] = v_view
    return out, grads
