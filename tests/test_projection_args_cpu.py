"""The nine projection entry points (array, splat rows, packed COO, fused dynamic slice) refuse bad calls before any launch, without
a GPU: for each one a well-formed argument list -- fake non-null pointers, never dereferenced -- with ONE thing broken at a time
must come back with a non-zero status and the message callers match on.  What is broken: each required pointer, both / neither of
covars and (quats, scales), camera_model -1 and 3 (every entry: an out-of-range model used to run as fisheye in the backward and
packed entries), and each entry's own checks (alignment, antialiased without opacities, SH degree / K, the shN mask, tiles, gradient
row strides, v_compensations without compensations, the quantizer tables).  An empty call returns 0 with every pointer null."""
import pytest

P = 1 << 16      # a fake pointer: non-null, 64-byte aligned, never dereferenced (every case is refused before the launch)
NULLPTR = "null pointer"
COVAR = "exactly one of covars / \\(quats, scales\\) must be given"
CAMERA = "bad camera_model"

SCALARS = dict(C=2, N=3, nnz=4, image_width=10, image_height=10, eps2d=0.3, near_plane=0.01, far_plane=1e10, radius_clip=0.0,
               camera_model=0, antialiased=1, sh_K=0, sh_degree=0, sh_mask_temperature=1.0, sh_mask_binary=0, tile_size=16, tile_width=1,
               tile_height=1, outputs_prefilled=1, v_means2d_stride=2, v_conics_stride=3, sparse_grad=0, timestamp=0.5, min_trbf=-1.0,
               raw_params=7, quant_mask=15)
# pointers that the well-formed call leaves out
ABSENT = ("covars", "sh_coeffs", "sh_coeffs_rest", "sh_mask_logits", "v_sh_coeffs", "v_sh_coeffs_rest", "v_sh_mask_logits", "v_covars", "stream")

SH = dict(colors=None, sh_coeffs=P, sh_K=4, sh_degree=1)                       # SH colours in the forward
SH_SPLIT = dict(SH, sh_coeffs_rest=P)
SH_BWD = dict(v_viewmats=None, v_colors=None, sh_coeffs=P, v_sh_coeffs=P, sh_K=4, sh_degree=1)  # the fused SH backward
SH_BWD_SPLIT = dict(SH_BWD, sh_coeffs_rest=P, v_sh_coeffs_rest=P)

# entry -> (required pointers, takes covars, sizes whose zero ends the call early, [(what is broken, message)] of its own checks)
ENTRIES = {
    "gs_projection_fwd": ("means viewmats Ks radii means2d depths conics", True, ("C", "N"), []),
    "gs_projection_rows_fwd": ("means viewmats Ks radii depths rows", True, ("C", "N"), [
        (dict(rows=P + 16), "the row buffer must be 64-byte aligned"),
        (dict(opacities=None), "antialiased needs the opacities"),
        (dict(sh_coeffs=P, sh_K=4, sh_degree=1), "colors and sh_coeffs exclude each other"),
        (dict(SH, sh_degree=5, sh_K=36), "bad SH degree / K"),
        (dict(SH, sh_degree=2), "bad SH degree / K"),
        (dict(sh_coeffs_rest=P), "sh_coeffs_rest needs sh_coeffs and K >= 2"),
        (dict(SH_SPLIT, sh_K=1, sh_degree=0), "sh_coeffs_rest needs sh_coeffs and K >= 2"),
        (dict(SH, sh_mask_logits=P), "the shN mask needs split coefficient rows"),
        (dict(SH_SPLIT, sh_mask_logits=P, sh_mask_temperature=0.0), "the mask temperature must be positive"),
        (dict(tiles_per_gauss=None), "block_sums come with tiles_per_gauss"),
        (dict(tile_size=0), "tile_size must be > 0"),
    ]),
    "gs_projection_rows_bwd": ("means viewmats Ks radii rows grad_rows", True, ("N",), [
        (dict(rows=P + 8), "row buffers must be 16-byte aligned"),
        (dict(grad_rows=P + 4), "row buffers must be 16-byte aligned"),
        (dict(opacities=None), "antialiased needs the opacities"),
        (dict(sh_mask_logits=P), "the shN mask needs the fused SH backward with split rows"),
        (dict(SH_BWD, sh_mask_logits=P), "the shN mask needs the fused SH backward with split rows"),
        (dict(SH_BWD_SPLIT, v_sh_mask_logits=P), "v_sh_mask_logits needs the \\(training-mode\\) mask"),
        (dict(SH_BWD_SPLIT, sh_mask_logits=P, sh_mask_binary=1, v_sh_mask_logits=P), "v_sh_mask_logits needs the \\(training-mode\\) mask"),
        (dict(SH_BWD, v_viewmats=P), "fused SH backward: no camera-pose / per-gaussian colour gradients"),
        (dict(SH_BWD, v_colors=P), "fused SH backward: no camera-pose / per-gaussian colour gradients"),
        (dict(SH_BWD, v_sh_coeffs=None), "fused SH backward: v_sh_coeffs, degree <= 4"),
        (dict(SH_BWD, sh_degree=5, sh_K=36), "fused SH backward: v_sh_coeffs, degree <= 4"),
        (dict(SH_BWD, sh_degree=2), "fused SH backward: v_sh_coeffs, degree <= 4"),
        (dict(SH_BWD, sh_coeffs_rest=P), "sh_coeffs_rest and v_sh_coeffs_rest go together"),
        (dict(SH_BWD, v_sh_coeffs_rest=P), "sh_coeffs_rest and v_sh_coeffs_rest go together"),
        (dict(SH_BWD, sh_K=9, sh_degree=2), "fused SH backward needs 3 K % 4 == 0"),
        (dict(SH_BWD, sh_coeffs=P + 4), "fused SH backward needs 3 K % 4 == 0"),
        (dict(SH_BWD, v_sh_coeffs=P + 8), "fused SH backward needs 3 K % 4 == 0"),
    ]),
    "gs_projection_bwd": ("means viewmats Ks radii conics v_means2d v_conics", True, ("N",), [
        (dict(v_means2d_stride=1), "bad gradient row strides"),
        (dict(v_conics_stride=2), "bad gradient row strides"),
        (dict(compensations=None), "v_compensations given without compensations"),
    ]),
    "gs_projection_packed_count": ("means viewmats Ks block_cnts", True, ("C", "N"), []),
    "gs_projection_packed_fill": ("means viewmats Ks block_accum indptr", True, ("C", "N"), []),
    "gs_projection_packed_bwd": ("means viewmats Ks camera_ids gaussian_ids conics v_means2d v_conics", True, ("nnz",), []),
    "gs_projection_rows_dyn_fwd": ("means quats scales motion omega trbf_center trbf_scale viewmats Ks radii depths rows", False, ("C", "N"), [
        (dict(rows=P + 32), "the row buffer must be 64-byte aligned"),
        (dict(opacities=None, quant_mask=11), "antialiased needs the opacities"),
        (dict(tiles_per_gauss=None), "block_sums come with tiles_per_gauss"),
        (dict(tile_size=0), "tile_size must be > 0"),
        (dict(opacities=None, antialiased=0), "quantized opacities need the opacities"),
        (dict(colors=None), "quantized colors need the colors"),
        (dict(quant_lo=None), "quant_mask set without the quantizer tables"),
        (dict(quant_step_norm=None, quant_mask=1), "quant_mask set without the quantizer tables"),
    ]),
    "gs_projection_rows_dyn_bwd": ("means quats scales motion omega trbf_center trbf_scale viewmats Ks radii rows grad_rows", False, ("N",), [
        (dict(rows=P + 8), "row buffers must be 16-byte aligned"),
        (dict(grad_rows=P + 4), "row buffers must be 16-byte aligned"),
        (dict(opacities=None), "the opacity / trbf gradients \\(and antialiased\\) need the opacities"),
        (dict(opacities=None, antialiased=0, v_opacities=None, v_trbf_center=None), "the opacity / trbf gradients"),
        (dict(quant_hi=None), "quant_mask set without the quantizer tables"),
    ]),
}


def good(name):
    """The well-formed argument list of an entry point, by parameter name (the names are the header's)."""
    from gscodec_studio_amd import _backend as B

    _, _, names = B.prototypes()[name]
    return {a: (SCALARS[a] if a in SCALARS else None if a in ABSENT else P) for a in names}


def refused(name, change, message):
    from gscodec_studio_amd import _backend as B

    args = good(name)
    assert set(change) <= set(args), (name, set(change) - set(args))
    args.update(change)
    with pytest.raises(RuntimeError, match=f"{name} failed \\(status [1-9]\\): {name}: {message}"):
        B.call(name, *args.values())


CASES = []
for _name, (_ptrs, _covars, _sizes, _own) in ENTRIES.items():
    CASES += [(_name, {p: None}, NULLPTR) for p in _ptrs.split()]
    if _covars:
        CASES += [(_name, dict(covars=P), COVAR), (_name, dict(quats=None, scales=None), COVAR), (_name, dict(quats=None), COVAR),
                  (_name, dict(scales=None), COVAR)]
    CASES += [(_name, dict(camera_model=-1), CAMERA), (_name, dict(camera_model=3), CAMERA)]
    CASES += [(_name, change, message) for change, message in _own]


def test_the_nine_entry_points_are_declared_and_exported():
    from gscodec_studio_amd import _backend as B

    assert len(ENTRIES) == 9
    for name, (ptrs, covars, sizes, _) in ENTRIES.items():
        names = B.prototypes()[name][2]
        assert hasattr(B.lib(), name) and set(ptrs.split()) | set(sizes) <= set(names) and ("covars" in names) == covars, name


@pytest.mark.parametrize("name,change,message", CASES, ids=[f"{n[3:]}-{'-'.join(f'{k}={v}' for k, v in c.items())}"[:96] for n, c, _ in CASES])
def test_one_thing_broken_is_refused_before_the_launch(name, change, message):
    refused(name, change, message)


@pytest.mark.parametrize("name", list(ENTRIES))
def test_an_empty_call_returns_zero_with_every_pointer_null(name):
    from gscodec_studio_amd import _backend as B

    for size in ENTRIES[name][2]:
        args = {a: (v if a in SCALARS else None) for a, v in good(name).items()}
        args[size] = 0
        B.call(name, *args.values())  # (a non-zero status raises)
