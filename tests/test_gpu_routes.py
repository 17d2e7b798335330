"""Which native entry points one ``rasterization()`` forward + ``loss.backward()`` goes through, per call shape: the routes
(step driver, splat rows through the operators, packed COO, fused / detoured dynamic slice, split / concatenated / masked SH
pair, the four SH evaluations) are host-side decisions, and the sequence of entry-point names is what they decide.  The table
below was recorded with this test body on the commit before the route decision moved into ``_route.py``."""
import pytest
import torch

from util import T, garden, garden_sh

pytestmark = pytest.mark.gpu

N_SPLATS, WIDTH, HEIGHT = 300, 48, 32  # two projection blocks; 3 x 2 tiles of 16 pixels
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


def run_case(colors, K=None, C=1, render_mode="RGB", packed=False, sparse_grad=False, covars=False, pose_grads=False, antialiased=False,
             absgrad=False, deterministic=False, channel_chunk=32, tile_size=16, dynamic=None, patch=None):
    """-> (entry-point names, render, alphas, meta, {name: gradient})"""
    import gscodec_studio_amd as G
    from gscodec_studio_amd import _backend, _readback, _step, _wrapper
    from gscodec_studio_amd.compression_simulation.ada_mask import MaskedShN
    from gscodec_studio_amd.dynamic import DynamicSlice

    g = garden(N_SPLATS, scale_mult=4.0)
    n = N_SPLATS
    gen = torch.Generator(device="cuda:0").manual_seed(3)

    def R(*shape):
        return torch.rand(shape, device="cuda:0", generator=gen)

    P = {"means": T(g["means"]), "opacities": T(g["opacities"])}
    if covars:
        c6, _ = _wrapper.quat_scale_to_covar_preci(T(g["quats"]), T(g["scales"]), compute_preci=False, triu=False)
        P["covars"] = c6.detach().clone()
    else:
        P["quats"], P["scales"] = T(g["quats"]), T(g["scales"])
    sh = garden_sh(g["rgb"], K=K) if K else None
    if colors == "n3":
        P["colors"] = T(g["rgb"])
    elif colors == "n5":
        P["colors"] = torch.cat([T(g["rgb"]), R(n, 2)], dim=1)
    elif colors == "cn3":
        P["colors"] = T(g["rgb"])[None].repeat(C, 1, 1) * R(C, 1, 1)
    elif colors == "sh":
        P["colors"] = T(sh)
    elif colors == "csh":
        P["colors"] = T(sh)[None].repeat(C, 1, 1, 1)
    else:
        P["sh0"] = T(sh[:, :1])
        P["shN"] = torch.cat([R(1), T(sh[:, 1:]).reshape(-1)]) if colors == "mask_view" else T(sh[:, 1:])
        if colors != "pair":
            P["mask_logits"] = (R(n, 1, 1) - 0.5) * 4
    dyn = None
    if dynamic:
        P.update(motion=0.02 * (R(n, 9) - 0.5), omega=0.1 * (R(n, 4) - 0.5), trbf_center=R(n, 1), trbf_scale=R(n, 1) + 0.5)
    vm = T(g["viewmats"][:C])
    Ks = g["Ks"][:C].copy()
    Ks[:, 0] *= WIDTH / g["width"]
    Ks[:, 1] *= HEIGHT / g["height"]
    Ks = T(Ks)
    if pose_grads:
        P["viewmats"] = vm
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
            P["means"], P.get("quats"), P.get("scales"), P["opacities"], col, vm, Ks, WIDTH, HEIGHT, sh_degree=int(K ** 0.5) - 1 if K else None,
            packed=packed, sparse_grad=sparse_grad, render_mode=render_mode, covars=P.get("covars"), absgrad=absgrad,
            rasterize_mode="antialiased" if antialiased else "classic", deterministic=deterministic, channel_chunk=channel_chunk,
            tile_size=tile_size, dynamic=dyn)
        meta["means2d"].retain_grad()
        weights = torch.rand(rc.shape, device="cuda:0", generator=gen)
        ((rc * weights).sum() + 0.5 * ra.sum()).backward()
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
    assert calls == EXPECTED[name].split()
    assert meta["flatten_ids"].numel() > 0 and float(ra.max()) > 0  # (the scene is visible: every stage had work)
    assert grads["means"] is not None and all(bool(torch.isfinite(v).all()) for v in grads.values() if v is not None)
