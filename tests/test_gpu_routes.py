"""``rasterization()`` forward + ``loss.backward()`` per call shape, over one table of 95 shapes (54 that choose a route, 41 that hold the
arguments every route has to carry): WHICH native entry points it goes through and WHAT it computes.

The routes (step driver, splat rows through the operators, packed COO, fused / detoured dynamic slice, split / concatenated / masked SH
pair, the four SH evaluations) are host-side decisions.  ``test_native_call_sequence`` holds the sequence of entry-point names they decide
(the table below was recorded with that test body on the commit before the route decision moved into ``_route.py``).
``test_route_values_against_float64`` holds the numbers: the image, the alphas, the projection outputs, the binning and every gradient of
the same run against tests/render_chain.py, the whole call evaluated on the CPU in float64 -- so that a route which reads the wrong buffer,
hands a cotangent to the wrong place, takes the wrong per-camera sum or renders the wrong channel as the depth fails, whatever its
kernels are called.  Both tests share one GPU run per case (``run_case`` is cached), and every case runs as it is: no extra determinism
switch, so that the path checked is the path used.

The bar is the one of tests/test_gpu_surfel.py: per quantity relative L2 against float64 <= max(1e-4, 4 e32), where e32 is the relative L2
of the SAME chain evaluated in float32 on the CPU against its float64 run -- what float32 arithmetic alone does to that quantity -- and the
factor 4 covers summation order and the hardware ``exp``; the forward outputs (image, alphas, ``means2d``, ``depths``, ``conics``) also largest entry error <= max(1e-4, 4 m32) of the largest
float64 entry.  Pixels where a compositing decision lies within a few ulp of flipping in either build get zero weight in the loss on both
sides -- the 0.5 x alphas term included, which a flipped decision moves like the image -- and are left out of the forward comparison (at most 2 %: tests/test_render_chain_cpu.py, which also holds identical radii of the two
builds and no SH colour at its clamp, for all 95 cases, on the reference alone).  ``radii`` equal the chain's; the binning equals the
oracle's on the call's own projection, bit for bit; rows of splats no camera sees are exactly zero; a tensor whose float64 gradient is
identically zero is zero or ``None``.  Every case prints one line per quantity with ``pytest -s``; the MI355X run is
profiles/routes_parity.txt.  Every case is expressed by the chain; none is held against a sibling instead.

Measured on the MI355X: on this scene the float32 chain is within 1.5e-5 of float64 in every quantity of every case (worst: ``means2d`` gradient
of the ED modes), so NO quantity rides on ``4 e32``: every bar of the table is the fixed 1e-4.  The kernels' worst is 1.7e-5 (the same
gradient, ratio 0.17); the image is within 9.5e-7 in relative L2 and 6.7e-6 in its largest entry (896 rows: 540 forward, 356 gradients).  Mutations that each failed value tests while every call sequence still passed: the
depth swapped with the blue channel in the packed RGB+D mode (``render`` and every gradient of packed-RGB+D), the SH gradient's sum over
cameras dropped (``colors`` / ``sh0`` / ``shN`` / ``mask_logits`` gradients of the two C = 2 shared-SH cases, 0.4 ... 0.6), the SH direction term left
out of ``v_means`` (``means`` gradient of 18 SH cases, 2e-3 ... 2e-2), the packed tile lists in gaussian order (``flatten_ids``, ``render``).

THE ARGUMENTS NO ROUTE DECISION READS.  ``_route.route()`` reads neither the camera model, the clip planes, ``radius_clip``, ``eps2d``, the
backgrounds nor ``sh_degree``; each route carries them to its own kernels (the fields of ``gs_step``, the arguments of ``project_rows``, of
the packed operators, of the dynamic kernels).  The 54 cases above hold all of them at their defaults, with every SH band active and hardly a
colour below its clamp.  41 more cases (``render_chain.BASE``: each is a case of the 54, its base, with keys changed) vary them per route:
``camera_model``, ``near_plane`` / ``far_plane``, ``radius_clip``, ``eps2d`` (to the call and to the chain), ``backgrounds`` (a ``[C,D]`` leaf whose
gradient joins the comparison; zero on a depth channel), ``tile_size=8`` on the step driver, ``deg`` (``sh_degree`` below the bands of K = 16: the
paths where the coefficient row is longer than the bands read -- the gradient of every band above it must be zero or ``None``, asserted band
by band) and ``sh_scale`` (bands >= 1 times 6, which puts 6 ... 14 % of the visible colours below the clamp: the gate of the SH backward, which
reads the forward's colours back at a stride that differs per route).  The bars are the table's own.  No option changes a route:
``test_native_call_sequence`` holds each of the 41 to the recorded sequence of its base, and on the MI355X all 41 equal it.  That every
option bites on this scene (pairs culled, radii and conics moved, colours clamped, a last active band with a gradient, a pixel that shows
the background) is asserted on the reference alone by tests/test_render_chain_cpu.py::test_no_option_case_is_vacuous.

Measured on the MI355X, the 41: 685 rows (410 forward, 275 gradients), the float32 chain within 2.5e-5 of float64 in every one of them, so NO new
quantity rides on ``4 e32`` either: every bar is the fixed 1e-4.  Worst 1.0e-5 (``means2d`` gradient of combined-sh16-RGB+ED-C2, ratio 0.10);
``grad backgrounds`` at most 5.8e-8.  Mutations, each on a copy of the tree, all 95 value tests run: the step driver entering pinhole whatever
``camera_model`` says (``radii`` of the 5 step-driver ortho / fisheye cases; the 54 pass), ``radius_clip`` passed as 0 to the packed projection
(``radii`` of packed-sh16-radius_clip; the 54 pass), the full degree in place of ``sh_degree`` in the step driver's forward (``render`` of 7 cases
with ``deg``, 2.6e-2 ... 6.7e-2; the 54 pass), ``alpha`` in place of ``1 - alpha`` in the background gradient (``grad backgrounds`` of all 8
backgrounds cases, 0.53 ... 0.77; the 54 pass), and the clamp gate of ``sh_bwd_lane`` removed: ``grad colors`` / ``sh0`` / ``shN`` / ``means`` of 18
new cases (0.46 on clamp-sh16 against 0.14 on rows-sh16) -- and of 21 of the 54, whose degree-3 scene has 11 of 597 colours below the clamp;
what the 54 do not see is the gate below degree 3 (step-sh16-deg0 / deg1 pass without it: no colour is clamped there), which
clamp-sh16-deg1 closes.
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import gs_oracle as O
from render_chain import BASE, CASES, CHAIN_OPTIONS, HEIGHT, N_SPLATS, WIDTH, render_chain, route_scene, sh_band, sh_degree_of
from util import N, T, rel_l2

pytestmark = pytest.mark.gpu

@functools.lru_cache(maxsize=None)
def _reference(key):
    """-> (scene, bool [C,H,W]: the pixels where neither build of the chain has a compositing decision near its threshold); one evaluation
    per set of inputs (``key``: the options of a case that choose an input, as sorted items), shared by ``run_case`` and the value test."""
    case = dict(key)
    scene = route_scene(**case)
    o32, _ = render_chain(32, case, scene=scene)
    o64, _ = render_chain(64, case, scene=scene)
    return scene, ~(o32["borderline"] | o64["borderline"])


_INPUT_KEYS = ("colors", "K", "C", "render_mode", "covars", "pose_grads", "antialiased", "tile_size", "dynamic", "packed", "camera_model",
               "near_plane", "far_plane", "radius_clip", "eps2d", "backgrounds", "deg", "sh_scale")
_DEFAULTS = dict(K=None, C=1, render_mode="RGB", covars=False, pose_grads=False, antialiased=False, tile_size=16, dynamic=None, packed=False,
                 backgrounds=False, deg=None, sh_scale=None, **CHAIN_OPTIONS)


def _input_key(case):
    return tuple((k, case.get(k, _DEFAULTS.get(k))) for k in _INPUT_KEYS)


def _cached(fn):
    memo = {}

    @functools.wraps(fn)
    def wrapper(*a, **kw):
        key = repr((a, sorted(kw.items())))
        if key not in memo:
            memo[key] = fn(*a, **kw)
        return memo[key]
    return wrapper


@_cached
def run_case(colors, K=None, C=1, render_mode="RGB", packed=False, sparse_grad=False, covars=False, pose_grads=False, antialiased=False,
             absgrad=False, deterministic=False, channel_chunk=32, tile_size=16, dynamic=None, patch=None, camera_model="pinhole",
             near_plane=0.01, far_plane=1e10, radius_clip=0.0, eps2d=0.3, backgrounds=False, deg=None, sh_scale=None):
    """-> (entry-point names, render, alphas, meta, {name: gradient}); one GPU run per call shape, shared by the tests of this module.
    The loss is (render * weights).sum() + 0.5 * alphas.sum() over the pixels that are not borderline."""
    import gscodec_studio_amd as G
    from gscodec_studio_amd import _backend, _readback, _step, _wrapper
    from gscodec_studio_amd.compression_simulation.ada_mask import MaskedShN
    from gscodec_studio_amd.dynamic import DynamicSlice

    S, ok = _reference(_input_key(dict(colors=colors, K=K, C=C, render_mode=render_mode, covars=covars, pose_grads=pose_grads,
                                       antialiased=antialiased, tile_size=tile_size, dynamic=dynamic, packed=packed,
                                       camera_model=camera_model, near_plane=near_plane, far_plane=far_plane, radius_clip=radius_clip,
                                       eps2d=eps2d, backgrounds=backgrounds, deg=deg, sh_scale=sh_scale)))
    n = N_SPLATS
    P = {k: T(v) for k, v in S["P"].items()}
    if backgrounds:
        P["backgrounds"] = T(S["backgrounds"])
    vm = P["viewmats"] if pose_grads else T(S["viewmats"])
    Ks = T(S["Ks"])
    dyn = None
    for p in P.values():
        p.requires_grad_(True)
    if dynamic:
        dyn = DynamicSlice(P["motion"], P["omega"], P["trbf_center"], P["trbf_scale"], 0.4,
                           quantize={"colors": (0.0, 1.0, 8)} if dynamic == "qcolors" else None)
    if "sh0" in P:
        shN = P["shN"][1:].view(n, K - 1, 3) if colors == "mask_view" else P["shN"]
        col = (P["sh0"], shN if colors == "pair" else MaskedShN(shN, P["mask_logits"], 0.7, False))
    else:
        col = P["colors"]
    calls = []
    real_call = _backend.call

    def recording_call(name, *a, **kw):
        calls.append(name)
        return real_call(name, *a, **kw)

    mods = {"_step": _step, "_wrapper": _wrapper, "_backend": _backend, "_readback": _readback}
    patches = dict(patch or {})
    patches["_backend", "call"] = recording_call
    saved = {k: getattr(mods[k[0]], k[1]) for k in patches}
    try:
        for k, v in patches.items():
            setattr(mods[k[0]], k[1], v)
        rc, ra, meta = G.rasterization(
            P["means"], P.get("quats"), P.get("scales"), P["opacities"], col, vm, Ks, WIDTH, HEIGHT, sh_degree=sh_degree_of(dict(K=K, deg=deg)),
            packed=packed, sparse_grad=sparse_grad, render_mode=render_mode, covars=P.get("covars"), absgrad=absgrad,
            rasterize_mode="antialiased" if antialiased else "classic", deterministic=deterministic, channel_chunk=channel_chunk,
            tile_size=tile_size, dynamic=dyn, camera_model=camera_model, near_plane=near_plane, far_plane=far_plane, radius_clip=radius_clip,
            eps2d=eps2d, backgrounds=P.get("backgrounds"))
        meta["means2d"].retain_grad()
        weights, mask = T(S["weights"] * ok[..., None]), T(ok[..., None].astype(np.float32))
        assert rc.shape == weights.shape, (rc.shape, weights.shape)
        ((rc * weights).sum() + 0.5 * (ra * mask).sum()).backward()
        torch.cuda.synchronize()
    finally:
        for k, v in saved.items():
            setattr(mods[k[0]], k[1], v)
    grads = {k: p.grad.to_dense() if p.grad is not None and p.grad.is_sparse else p.grad for k, p in P.items()}
    grads["means2d"] = meta["means2d"].grad
    if absgrad:
        grads["absgrad"] = meta["means2d"].absgrad
    return calls, rc.detach(), ra.detach(), meta, grads


EXPECTED = {
    'rows-RGB':
        'gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd gs_projection_rows_bwd',
    'rows-D':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_isect_finish_presorted'
        ' gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_projection_rows_bwd',
    'rows-ED':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_isect_finish_presorted'
        ' gs_rasterize_plan gs_rasterize_fwd gs_expected_depth_fwd gs_expected_depth_bwd gs_rasterize_bwd gs_projection_rows_bwd',
    'rows-RGB+D':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_isect_finish_presorted'
        ' gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_projection_rows_bwd',
    'rows-RGB+ED':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_isect_finish_presorted'
        ' gs_rasterize_plan gs_rasterize_fwd gs_expected_depth_fwd gs_expected_depth_bwd gs_rasterize_bwd gs_projection_rows_bwd',
    'packed-RGB':
        'gs_projection_packed_count gs_cumsum_i32_i32 gs_projection_packed_fill gs_gather_rows_f32 gs_presort_split'
        ' gs_isect_count_keys gs_presort_buckets gs_gather_rows_f32 gs_isect_finish_presorted gs_rasterize_plan gs_rasterize_fwd'
        ' gs_rasterize_bwd gs_scatter_add_rows_f32 gs_scatter_add_rows_f32 gs_projection_packed_bwd',
    'packed-D':
        'gs_projection_packed_count gs_cumsum_i32_i32 gs_projection_packed_fill gs_gather_rows_f32 gs_presort_split'
        ' gs_isect_count_keys gs_presort_buckets gs_gather_rows_f32 gs_isect_finish_presorted gs_rasterize_plan gs_rasterize_fwd'
        ' gs_rasterize_bwd gs_scatter_add_rows_f32 gs_projection_packed_bwd',
    'packed-ED':
        'gs_projection_packed_count gs_cumsum_i32_i32 gs_projection_packed_fill gs_gather_rows_f32 gs_presort_split'
        ' gs_isect_count_keys gs_presort_buckets gs_gather_rows_f32 gs_isect_finish_presorted gs_rasterize_plan gs_rasterize_fwd'
        ' gs_expected_depth_fwd gs_expected_depth_bwd gs_rasterize_bwd gs_scatter_add_rows_f32 gs_projection_packed_bwd',
    'packed-RGB+D':
        'gs_projection_packed_count gs_cumsum_i32_i32 gs_projection_packed_fill gs_gather_rows_f32 gs_presort_split'
        ' gs_isect_count_keys gs_presort_buckets gs_gather_rows_f32 gs_isect_finish_presorted gs_rasterize_plan gs_rasterize_fwd'
        ' gs_rasterize_bwd gs_scatter_add_rows_f32 gs_scatter_add_rows_f32 gs_projection_packed_bwd',
    'packed-RGB+ED':
        'gs_projection_packed_count gs_cumsum_i32_i32 gs_projection_packed_fill gs_gather_rows_f32 gs_presort_split'
        ' gs_isect_count_keys gs_presort_buckets gs_gather_rows_f32 gs_isect_finish_presorted gs_rasterize_plan gs_rasterize_fwd'
        ' gs_expected_depth_fwd gs_expected_depth_bwd gs_rasterize_bwd gs_scatter_add_rows_f32 gs_scatter_add_rows_f32'
        ' gs_projection_packed_bwd',
    'rows-n5':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_isect_finish_presorted'
        ' gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_projection_rows_bwd',
    'rows-cn3':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_isect_finish_presorted'
        ' gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_projection_rows_bwd',
    'packed-n5':
        'gs_projection_packed_count gs_cumsum_i32_i32 gs_projection_packed_fill gs_gather_rows_f32 gs_presort_split'
        ' gs_isect_count_keys gs_presort_buckets gs_gather_rows_f32 gs_isect_finish_presorted gs_rasterize_plan gs_rasterize_fwd'
        ' gs_rasterize_bwd gs_scatter_add_rows_f32 gs_scatter_add_rows_f32 gs_projection_packed_bwd',
    'packed-cn3':
        'gs_projection_packed_count gs_cumsum_i32_i32 gs_projection_packed_fill gs_gather_rows_f32 gs_presort_split'
        ' gs_isect_count_keys gs_presort_buckets gs_isect_finish_presorted gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd'
        ' gs_scatter_add_rows_f32 gs_projection_packed_bwd',
    'rows-sh4':
        'gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd gs_projection_rows_bwd',
    'rows-sh9':
        'gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd gs_sh_view_bwd'
        ' gs_projection_rows_bwd',
    'rows-sh16':
        'gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd gs_projection_rows_bwd',
    'rows-csh4':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_camera_centers gs_sh_fwd'
        ' gs_isect_finish_presorted gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_sh_bwd gs_projection_rows_bwd',
    'rows-csh9':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_camera_centers gs_sh_fwd'
        ' gs_isect_finish_presorted gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_sh_bwd gs_projection_rows_bwd',
    'rows-csh16':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_camera_centers gs_sh_fwd'
        ' gs_isect_finish_presorted gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_sh_bwd gs_projection_rows_bwd',
    'rows-pair4':
        'gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd gs_projection_rows_bwd',
    'rows-pair9':
        'gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd gs_sh_view_bwd'
        ' gs_projection_rows_bwd',
    'rows-pair16':
        'gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd gs_projection_rows_bwd',
    'packed-sh16':
        'gs_projection_packed_count gs_cumsum_i32_i32 gs_projection_packed_fill gs_gather_rows_f32 gs_presort_split'
        ' gs_isect_count_keys gs_presort_buckets gs_camera_centers gs_gather_rows_f32 gs_gather_rows_f32 gs_sh_fwd'
        ' gs_isect_finish_presorted gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_sh_bwd gs_scatter_add_rows_f32'
        ' gs_scatter_add_rows_f32 gs_scatter_add_rows_f32 gs_projection_packed_bwd',
    'packed-csh16':
        'gs_projection_packed_count gs_cumsum_i32_i32 gs_projection_packed_fill gs_gather_rows_f32 gs_presort_split'
        ' gs_isect_count_keys gs_presort_buckets gs_camera_centers gs_gather_rows_f32 gs_sh_fwd gs_isect_finish_presorted'
        ' gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_sh_bwd gs_scatter_add_rows_f32 gs_scatter_add_rows_f32'
        ' gs_projection_packed_bwd',
    'packed-pair16':
        'gs_projection_packed_count gs_cumsum_i32_i32 gs_projection_packed_fill gs_gather_rows_f32 gs_presort_split'
        ' gs_isect_count_keys gs_presort_buckets gs_camera_centers gs_gather_rows_f32 gs_gather_rows_f32 gs_sh_fwd'
        ' gs_isect_finish_presorted gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_sh_bwd gs_scatter_add_rows_f32'
        ' gs_scatter_add_rows_f32 gs_scatter_add_rows_f32 gs_projection_packed_bwd',
    'mask4':
        'gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd gs_projection_rows_bwd',
    'mask9':
        'gs_shn_mask_fwd gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd'
        ' gs_sh_view_bwd gs_projection_rows_bwd gs_shn_mask_bwd',
    'mask16':
        'gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd gs_projection_rows_bwd',
    'mask16-view':
        'gs_shn_mask_fwd gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd'
        ' gs_projection_rows_bwd gs_shn_mask_bwd',
    'mask16-C2':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_isect_finish_presorted'
        ' gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_projection_rows_bwd',
    'packed-sparse_grad':
        'gs_projection_packed_count gs_cumsum_i32_i32 gs_projection_packed_fill gs_gather_rows_f32 gs_presort_split'
        ' gs_isect_count_keys gs_presort_buckets gs_gather_rows_f32 gs_isect_finish_presorted gs_rasterize_plan gs_rasterize_fwd'
        ' gs_rasterize_bwd gs_scatter_add_rows_f32 gs_scatter_add_rows_f32 gs_projection_packed_bwd',
    'covars':
        'gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd gs_projection_rows_bwd',
    'pose-sh16':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_sh_fwd gs_isect_finish_presorted'
        ' gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_sh_bwd gs_projection_rows_bwd',
    'pose-pair16':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_sh_fwd gs_isect_finish_presorted'
        ' gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_sh_bwd gs_projection_rows_bwd',
    'pose-n3':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_isect_finish_presorted'
        ' gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_projection_rows_bwd',
    'antialiased-sh16':
        'gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd gs_projection_rows_bwd',
    'antialiased-packed':
        'gs_projection_packed_count gs_cumsum_i32_i32 gs_projection_packed_fill gs_gather_rows_f32 gs_presort_split'
        ' gs_isect_count_keys gs_presort_buckets gs_camera_centers gs_gather_rows_f32 gs_gather_rows_f32 gs_sh_fwd'
        ' gs_isect_finish_presorted gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_sh_bwd gs_scatter_add_rows_f32'
        ' gs_scatter_add_rows_f32 gs_scatter_add_rows_f32 gs_projection_packed_bwd',
    'absgrad':
        'gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd gs_projection_rows_bwd',
    'deterministic':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_isect_finish_presorted'
        ' gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_projection_rows_bwd',
    'channel_chunk2':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_isect_finish_presorted'
        ' gs_rasterize_plan gs_rasterize_fwd gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_rasterize_bwd'
        ' gs_projection_rows_bwd',
    'tile32':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_isect_finish_presorted'
        ' gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_projection_rows_bwd',
    'rows-sh16-RGB+ED-C2':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_isect_finish_presorted'
        ' gs_rasterize_plan gs_rasterize_fwd gs_expected_depth_fwd gs_expected_depth_bwd gs_rasterize_bwd gs_projection_rows_bwd',
    'dynamic-fused':
        'gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd gs_projection_rows_dyn_bwd',
    'dynamic-fused-qcolors':
        'gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd gs_projection_rows_dyn_bwd',
    'dynamic-detour-qcolors-n5':
        'gs_quantize_round_fwd gs_temporal_slice_fwd gs_projection_rows_fwd gs_presort_split gs_isect_count_keys'
        ' gs_presort_buckets gs_isect_finish_presorted gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_projection_rows_bwd'
        ' gs_temporal_slice_bwd',
    'dynamic-detour-sh16':
        'gs_temporal_slice_fwd gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd'
        ' gs_projection_rows_bwd gs_temporal_slice_bwd',
    'step-off-sh16':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_isect_finish_presorted'
        ' gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_projection_rows_bwd',
    'step-off-n3':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_isect_finish_presorted'
        ' gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_projection_rows_bwd',
    'two-launch-sh-bwd':
        'gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd gs_sh_view_bwd'
        ' gs_projection_rows_bwd',
    'two-launch-sh-bwd-mask16':
        'gs_shn_mask_fwd gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd'
        ' gs_sh_view_bwd gs_projection_rows_bwd gs_shn_mask_bwd',
    'prefill-off':
        'gs_step_fwd_begin gs_step_fwd_finish gs_rasterize_plan gs_step_fwd_finish gs_rasterize_bwd gs_projection_rows_bwd',
    'prefill-off-operators':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_isect_finish_presorted'
        ' gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_projection_rows_bwd',
    'pinned-direct-max-0':
        'gs_projection_rows_fwd gs_presort_split gs_isect_count_keys gs_presort_buckets gs_isect_finish_presorted'
        ' gs_rasterize_plan gs_rasterize_fwd gs_rasterize_bwd gs_projection_rows_bwd',
}


@pytest.mark.parametrize("name", list(CASES))
def test_native_call_sequence(name):
    calls, rc, ra, meta, grads = run_case(**CASES[name])
    assert calls == EXPECTED[BASE.get(name, name)].split()  # (an option, a lower sh_degree or other coefficients change no route)
    assert meta["flatten_ids"].numel() > 0 and float(ra.max()) > 0  # (the scene is visible: every stage had work)
    assert grads["means"] is not None and all(bool(torch.isfinite(v).all()) for v in grads.values() if v is not None)


def _bar(e32):
    return max(1e-4, 4.0 * e32)


def _dense(meta, key, C):
    """A projection output of the call as numpy [C,N,...]: packed routes scatter their (camera_ids, gaussian_ids) form."""
    v = N(meta[key]) if torch.is_tensor(meta[key]) else np.asarray(meta[key])
    if meta["camera_ids"] is None:
        return v
    out = np.zeros((C, N_SPLATS) + v.shape[1:], v.dtype)
    out[N(meta["camera_ids"]), N(meta["gaussian_ids"])] = v
    return out


def _per_splat(colors, key, g):
    """A gradient as [N, ...] rows, one per splat (None: not a per-splat tensor)."""
    if key in ("viewmats", "backgrounds", "means2d", "absgrad"):
        return None
    if key == "colors" and colors in ("cn3", "csh"):
        return np.moveaxis(g, 0, 1)
    if key == "shN" and colors == "mask_view":
        return g[1:].reshape(N_SPLATS, -1)
    return g


@pytest.mark.parametrize("name", list(CASES))
def test_route_values_against_float64(name):
    case = CASES[name]
    calls, rc, ra, meta, grads = run_case(**case)
    S, ok = _reference(_input_key(case))
    print()  # (the table starts on a line of its own, not behind pytest's progress dot)
    C, ts = S["viewmats"].shape[0], case.get("tile_size", 16)
    w = S["weights"] * ok[..., None]
    a = 0.5 * ok[..., None]
    o64, g64 = render_chain(64, case, cot=dict(render=w, alphas=a), scene=S)
    o32, g32 = render_chain(32, case, cot=dict(render=w, alphas=a.astype(np.float32)), scene=S)
    rows, failures = [], []

    def hold(quantity, hip, f32, f64, max_norm=False):
        hip, f32, f64 = (np.asarray(v, np.float64) for v in (hip, f32, f64))
        assert hip.shape == f64.shape, (quantity, hip.shape, f64.shape)
        checks = [("l2", rel_l2(hip, f64), _bar(rel_l2(f32, f64)))]
        if max_norm:
            top = np.abs(f64).max()
            checks.append(("max", np.abs(hip - f64).max() / top, _bar(np.abs(f32 - f64).max() / top)))
        for kind, err, bar in checks:
            row = f"[routes] {name:28s} {quantity:18s} {kind:3s} err {err:.3e}  bar {bar:.3e}  ratio {err / bar:.3f}"
            print(row)
            rows.append(row)
            if not err <= bar:
                failures.append(row)

    # ---- forward: the image and the alphas where not borderline
    m = ok[..., None]
    assert tuple(rc.shape) == o64["render"].shape and tuple(ra.shape) == o64["alphas"].shape
    hold("render", N(rc) * m, o32["render"] * m, o64["render"] * m, max_norm=True)
    hold("alphas", N(ra) * m, o32["alphas"] * m, o64["alphas"] * m, max_norm=True)

    # ---- the projection where visible
    radii = _dense(meta, "radii", C)
    assert np.array_equal(radii, o64["radii"]) and np.array_equal(o32["radii"], o64["radii"]), "radii differ from the chain's"
    vis = radii > 0
    for k in ("means2d", "depths", "conics"):
        v = _dense(meta, k, C)
        sel = vis.reshape(vis.shape + (1,) * (v.ndim - 2))
        hold(k, np.where(sel, v, 0), np.where(sel, o32[k], 0), np.where(sel, o64[k], 0), max_norm=True)

    # ---- the binning, bit for bit, on the call's own projection
    tw, th = math.ceil(WIDTH / ts), math.ceil(HEIGHT / ts)
    packed = meta["camera_ids"] is not None
    o_tpg, o_ids, o_flat = O.isect_tiles(N(meta["means2d"]), N(meta["radii"]), N(meta["depths"]), ts, tw, th, n_cameras=C,
                                         camera_ids=N(meta["camera_ids"]) if packed else None)
    assert np.array_equal(N(meta["tiles_per_gauss"]), o_tpg), "tiles_per_gauss"
    assert np.array_equal(N(meta["flatten_ids"]), o_flat), "flatten_ids"
    assert np.array_equal(N(meta["isect_offsets"]), O.isect_offset_encode(o_ids, C, tw, th)), "isect_offsets"

    # ---- every gradient
    assert set(S["P"]) <= set(grads) and set(S["P"]) <= set(g64)
    unseen = ~vis.any(0)
    assert unseen.any() and not unseen.all()
    if case.get("deg") is not None:  # the bands above sh_degree: identically zero in float64, so zero or None here, band by band
        for b in range(case["deg"] + 1, int(case["K"] ** 0.5)):
            k, idx = sh_band(case["colors"], b)
            assert not g64[k][idx].any() and not g32[k][idx].any(), (k, b)
            assert grads[k] is None or not N(grads[k])[idx].any(), (k, b, "the float64 gradient of this band is identically zero")
    for k in list(S["P"]) + (["backgrounds"] if case.get("backgrounds") else []) + ["means2d"] + (["absgrad"] if case.get("absgrad") else []):
        h = grads[k]
        if not g64[k].any():  # (colours in a depth-only mode)
            assert h is None or not bool(h.any()), (k, "the float64 gradient is identically zero")
            continue
        assert h is not None, k
        h = _dense({**meta, k: h}, k, C) if k in ("means2d", "absgrad") else N(h)
        a32, a64 = g32[k], g64[k]
        if k == "viewmats":
            assert not h[:, 3].any(), "the bottom row of v_viewmats stays zero"
            h, a32, a64 = h[:, :3], a32[:, :3], a64[:, :3]
        if k in ("means2d", "absgrad"):
            assert not h[~vis].any(), (k, "entries of pairs that are not visible are exactly zero")
        per = _per_splat(case["colors"], k, h)
        if per is not None:
            assert not per[unseen].any(), (k, "rows of splats no camera sees are exactly zero")
        hold("grad " + k, h, a32, a64)
    assert not failures, "\n".join(failures)
