/*
 * gsplat_hip.h -- flat C ABI of libgsplat_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for the rasterize + quantize hot path of
 * JasonLSC/GSCodec_Studio (a gsplat 1.4.0 fork).  Every entry point replaces one
 * pybind11 function of the reference's native module (reference file:line cited
 * per function, paths relative to the reference root).  Differences from the
 * reference's native surface, all deliberate:
 *
 *   - no torch types: raw device pointers + explicit sizes + a hipStream_t
 *     (passed as void*), so any host (ctypes, cgo, JNI, a C++ runtime) can bind it;
 *   - the CALLER owns every buffer, including scratch; the library keeps no
 *     global device state and never allocates or frees device memory;
 *   - data-dependent sizes (n_isects, nnz) use a two-call protocol: a *_count
 *     call leaves the total in caller memory, the caller allocates, then calls
 *     the *_emit / *_fill entry point;
 *   - every function returns 0 on success, non-zero on error; the message is
 *     available (thread-local) from gs_last_error().  Nothing throws or aborts
 *     across the ABI;
 *   - all launches are asynchronous on the given stream.
 *
 * All floating-point tensors are fp32, contiguous, row-major.  Integer dtypes
 * match the reference's meta tensors (radii/flatten_ids/offsets/last_ids int32,
 * isect_ids/camera_ids/gaussian_ids int64, masks uint8/bool).
 */
#ifndef GSPLAT_HIP_H
#define GSPLAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an exported signature or the meaning of an argument changes (1: round 1; 2: the round-2 additions to
 * gs_rasterize_fwd, gs_isect_count_keys, gs_sort_pairs_u64_i32_drop, gs_projection_bwd; 3: round 3 -- the splat-row layout,
 * gs_raster_plan, gs_kmeans_decode's bounds; 4: round 4 -- the shN mask entry points, gs_isect_count_keys' bucket_splitters, the bucketed pre-sort; 5: round 6 -- gs_projection_rows_dyn_*, the dyn_* fields of gs_step, gs_accumulate_*, gs_quantize_round_multi_*, the scratch behind gs_presort_split's table; 6: the step driver's backward entry point and the backward fields of gs_step removed).  A binding must refuse a library whose gs_version() differs from the
 * GS_ABI_VERSION of the header it was generated from, and SHOULD also compare gs_header_hash() (the first 8 bytes of the
 * SHA-256 of the header file the library was compiled against, big-endian) with the hash of its own copy: ctypes / cgo call
 * through shifted argument lists silently otherwise.
 * ABI 6 later gained the optimizer entries (gs_adam_desc, gs_adam_multi, gs_adam_multi_max, gs_adam_desc_layout) and the loss
 * entries (gs_ssim_fwd, gs_ssim_bwd, gs_ssim_work_bytes, gs_ssim_window): additive, no existing signature changed.  The
 * densification-strategy entries (gs_relocation, gs_inject_noise, gs_densify_stats) are additive in the same way, and so are
 * the two of the spacetime strategies (gs_stg_omega_mask, gs_stg_freeze_grads), and the bilateral-grid entries
 * (gs_bilagrid_slice_fwd / _bwd, gs_bilagrid_tv_fwd / _bwd, gs_bilagrid_tv_work_bytes), and the entropy-coder entries
 * (gs_ans_histogram, gs_ans_encode_bytes, gs_ans_encode, gs_ans_pack, gs_ans_decode), and the grid-sort entries
 * (gs_gridsort_blur, gs_gridsort_keys, gs_gridsort_assign), and the 2D Gaussian splatting entries (gs_projection_2dgs_fwd / _bwd,
 * gs_rasterize_2dgs_fwd / _bwd, gs_depth_to_normal_fwd / _bwd), and the spacetime colour decoder's (gs_stg_decode_fwd / _bwd,
 * gs_stg_decode_partial_rows), and the appearance module's (gs_appearance_fwd / _bwd, gs_appearance_partial_rows,
 * gs_appearance_partial_cols), and the K-means entries (gs_kmeans_padded_width, gs_kmeans_default_slices, gs_kmeans_assign,
 * gs_kmeans_update), and the nearest-neighbour entries (gs_knn_cells, gs_knn_finish_grid, gs_knn_search), and the
 * PLY entries (gs_ply_unpack, gs_ply_pack, gs_ply_max_stride, gs_ply_max_columns, gs_ply_block_rows), and the hash-grid Gaussian entropy model's (gs_hashgrid_encode_fwd / _bwd,
 * gs_gaussian_bits_fwd / _bwd), and the Gaussian entropy coder's (gs_ans_pack_slots, gs_gauss_ans_slot_bytes,
 * gs_gauss_ans_encode_bytes, gs_gauss_ans_params, gs_gauss_ans_encode, gs_gauss_ans_decode), and the SparseAdam entries
 * (gs_sparse_adam_desc, gs_sparse_adam_multi, gs_sparse_adam_desc_layout), and the colour-matching entries
 * (gs_color_correct_pass, gs_color_correct_solve, gs_color_correct_record_doubles, gs_color_correct_rcond_log2), and the plane codec's (gs_plane_transform_fwd / _inv,
 * gs_plane_ans_slot_bytes, gs_plane_ans_encode, gs_plane_ans_decode), and the plane-sequence codec's (gs_plane_seq_fwd,
 * gs_plane_seq_inv). */
#define GS_ABI_VERSION 6

/* reference: gsplat/cuda/include/bindings.h:34-38 (enum CameraModelType) */
#define GS_CAMERA_PINHOLE 0
#define GS_CAMERA_ORTHO 1
#define GS_CAMERA_FISHEYE 2

/* quantizer modes (reference: gsplat/compression_simulation/ops.py:39-54) */
#define GS_QUANT_NOISE 0
#define GS_QUANT_ROUND 1
/* activation fused behind a quantizer (opt-in; 0 keeps the reference's bit-exact output) */
#define GS_ACT_NONE 0
#define GS_ACT_EXP 1
#define GS_ACT_SIGMOID 2

typedef void *gs_stream_t; /* hipStream_t */

int32_t gs_version(void);
uint64_t gs_header_hash(void);
const char *gs_last_error(void);

/* ------------------------------------------------------------------------
 * Splat rows: ONE 64-byte row of 16 floats per projected splat (camera, gaussian), the layout the compositing kernels
 * fetch with a single L2 request (three 16-byte loads from one line) instead of four gathers from four arrays:
 *   [0] mean2d.x  [1] mean2d.y  [2] conic.a  [3] conic.b  [4] conic.c  [5] opacity (after antialias compensation)
 *   [6] [7] [8] colour            [9] depth   [10] radius (int32 bit pattern)   [11] compensation   [12..15] reserved
 * The reference's tensors (means2d [C,N,2], conics [C,N,3], opacities [C,N], colours [C,N,3]; gsplat/rendering.py:337-349)
 * are COLUMN VIEWS of the row buffer, so `meta` keeps its keys, shapes and dtypes.  gs_projection_rows_fwd fills
 * columns 0-5 and 9-11 (and 6-8 for post-activation colours), gs_sh_view_fwd columns 6-8.  Rows of culled splats
 * (radii == 0) are left untouched, as the reference leaves means2d / conics uninitialised there.  The gradient rows the
 * compositing backward accumulates into (gs_rasterize_bwd, packed16) use the same columns: v_mean2d | v_conic |
 * v_opacity | v_colour (4 channels: column 9 is the fourth) | [10] [11] absgrad.
 * ---------------------------------------------------------------------- */
#define GS_ROW_FLOATS 16
#define GS_ROW_MEAN2D 0
#define GS_ROW_CONIC 2
#define GS_ROW_OPACITY 5
#define GS_ROW_COLOR 6
#define GS_ROW_DEPTH 9
#define GS_ROW_RADIUS 10
#define GS_ROW_COMPENSATION 11


/* ------------------------------------------------------------------------
 * R1  fully fused projection
 * replaces fully_fused_projection_fwd_tensor
 *   (gsplat/cuda/csrc/fully_fused_projection_fwd.cu:198-275, kernel 22-196)
 * Exactly one of {covars} / {quats, scales} is non-NULL.
 * Outputs for entries with radii == 0 are left untouched (the reference leaves
 * them uninitialised); compensations (optional) must be zero-filled by the caller.
 * ---------------------------------------------------------------------- */
int32_t gs_projection_fwd(
    uint32_t C, uint32_t N,
    const float *means,    /* [N,3] */
    const float *covars,   /* [N,6] triu or NULL */
    const float *quats,    /* [N,4] wxyz or NULL */
    const float *scales,   /* [N,3] or NULL */
    const float *viewmats, /* [C,4,4] world->camera */
    const float *Ks,       /* [C,3,3] */
    int32_t image_width, int32_t image_height,
    float eps2d, float near_plane, float far_plane, float radius_clip,
    int32_t camera_model,
    int32_t *radii,       /* [C,N] */
    float *means2d,       /* [C,N,2] */
    float *depths,        /* [C,N] */
    float *conics,        /* [C,N,3] */
    float *compensations, /* [C,N] or NULL */
    gs_stream_t stream);

/* replaces fully_fused_projection_bwd_tensor
 *   (gsplat/cuda/csrc/fully_fused_projection_bwd.cu:265-372, kernel 24-263)
 * v_means / v_covars / v_quats / v_scales are fully OVERWRITTEN (one thread owns one
 * gaussian and sums over cameras in registers: no atomics, deterministic).
 * v_viewmats (optional) is ACCUMULATED with atomics: caller zero-fills it. */
int32_t gs_projection_bwd(
    uint32_t C, uint32_t N,
    const float *means, const float *covars, const float *quats, const float *scales,
    const float *viewmats, const float *Ks,
    int32_t image_width, int32_t image_height, float eps2d, int32_t camera_model,
    const int32_t *radii,        /* [C,N] */
    const float *conics,         /* [C,N,3] */
    const float *compensations,  /* [C,N] or NULL */
    const float *v_means2d,      /* [C,N,2] */
    const float *v_depths,       /* [C,N] or NULL (= zero) */
    const float *v_conics,       /* [C,N,3] */
    const float *v_compensations,/* [C,N] or NULL */
    float *v_means,   /* [N,3] or NULL */
    float *v_covars,  /* [N,6] or NULL */
    float *v_quats,   /* [N,4] or NULL */
    float *v_scales,  /* [N,3] or NULL */
    float *v_viewmats,/* [C,4,4] or NULL */
    uint32_t v_means2d_stride, /* row stride of v_means2d in floats: 2, or 16 for the packed compositing rows */
    uint32_t v_conics_stride,  /* row stride of v_conics in floats: 3, or 16 */
    const float *v_means_add,  /* [N,3] or NULL: added to v_means (the d/d means that arrives through the SH view
                                  directions, rendering.py:381-391 in the reference; saves autograd's elementwise sum) */
    gs_stream_t stream);

/* Row form of the fused projection (what rasterization() uses for unpacked batches): same arithmetic and culling as
 * gs_projection_fwd, but every visible (camera, gaussian) pair gets ONE splat row (see "Splat rows" above) instead of
 * entries in three arrays.  Folded in, because the row wants them and the pass runs anyway:
 *   opacities [N] (or NULL): column 5 = opacities[n]              -- the `opacities.repeat(C, 1)` of rendering.py:331,
 *                            x compensation when antialiased != 0  -- and the multiply of rendering.py:334-335;
 *   colors [N,3] (or NULL):  columns 6-8 = colors[n]               -- the `colors.expand(C, -1, -1)` of rendering.py:386;
 *   sh_coeffs [N,sh_K,3] (or NULL; excludes colors): columns 6-8 = max(SH(means[n] - camera centre) + 0.5, 0) for the
 *                            first (sh_degree + 1)^2 bands -- exactly what gs_sh_view_fwd writes (same arithmetic, bit for
 *                            bit), without its launch and its second pass over means / radii; its gradient stays with
 *                            gs_sh_view_bwd.
 * radii [C,N] and depths [C,N] are ALSO written densely (the binning kernels stream through them); rows must be 64-byte
 * aligned; rows / depths of culled pairs are left untouched. */
int32_t gs_projection_rows_fwd(
    uint32_t C, uint32_t N,
    const float *means, const float *covars, const float *quats, const float *scales,
    const float *viewmats, const float *Ks,
    int32_t image_width, int32_t image_height,
    float eps2d, float near_plane, float far_plane, float radius_clip,
    int32_t camera_model,
    const float *opacities, const float *colors, int32_t antialiased,
    const float *sh_coeffs, const float *sh_coeffs_rest /* NULL or split rows, as in gs_sh_view_fwd */, uint32_t sh_K,
    uint32_t sh_degree,
    const float *sh_mask_logits /* NULL, or [N] (split rows only): the shN mask of the compression-simulation hooks
                                   (gs_shn_mask_fwd) applied on the fly -- the coefficients of the bands >= 1 are
                                   multiplied by sigmoid(logit / temperature) (binary: sigmoid(logit) >= 0.5) as they are
                                   loaded, the masked coefficients are never materialised; bit-identical to masking first */,
    float sh_mask_temperature, int32_t sh_mask_binary,
    uint32_t tile_size, uint32_t tile_width, uint32_t tile_height,
    int32_t *tiles_per_gauss /* NULL, or [C,N]: the binning's tile count of every pair (gs_isect_count), in the same pass */,
    int32_t *block_sums /* NULL, or [C * gs_projection_rows_blocks(N)][2] (8-byte aligned; may be pinned host memory): per
                           workgroup (sum of the counts, number of visible pairs), written as ONE 8-byte store -- the totals
                           are n_isects and the number of elements the depth pre-sort keeps, known to the host one kernel into
                           the step (the read-back of isect_tiles.cu:200) while the whole depth pre-sort is still queued;
                           gs_isect_count_keys then takes means2d = NULL, block_sums = NULL (tiles_per_gauss is an input there) */,
    int32_t *radii, /* [C,N] */
    float *depths,  /* [C,N] */
    float *rows,    /* [C,N,16] */
    gs_stream_t stream);
uint32_t gs_projection_rows_blocks(uint32_t N);
/* Its backward: grad_rows [C,N,16] holds d/d(mean2d, conic, opacity, colour) in the splat-row columns (what gs_rasterize_bwd
 * accumulates with packed16), v_depths [C,N] or NULL.  Besides the outputs of gs_projection_bwd (all OVERWRITTEN),
 * v_opacities [N] = sum over cameras of column 5 (x compensation when antialiased, whose own gradient then enters the
 * projection chain) and v_colors [N,3] = sum over cameras of columns 6-8; either may be NULL.
 * outputs_prefilled != 0: the caller guarantees that every per-gaussian output already holds zeros (e.g. through the
 * zero_fill of gs_rasterize_fwd); the rows of gaussians that no camera sees (71 % at BASELINE config 2) are then not
 * written at all, and v_means_add is only read where some camera sees the gaussian.
 * sh_coeffs != NULL (the forward evaluated the colours from them): the SH backward of gs_sh_view_bwd runs IN THE SAME PASS --
 * v_sh_coeffs [N,K,3] (or the pair v_sh_coeffs [N,1,3] / v_sh_coeffs_rest [N,K-1,3] for split coefficients) is written, and
 * the gradient that reaches the means through the view directions is added to v_means without leaving the lane.  Needs
 * 3 K % 4 == 0, 16-byte aligned coefficient / gradient rows, v_viewmats == NULL and v_colors == NULL; otherwise call
 * gs_sh_view_bwd first and hand its v_means over as v_means_add. */
int32_t gs_projection_rows_bwd(
    uint32_t C, uint32_t N,
    const float *means, const float *covars, const float *quats, const float *scales,
    const float *viewmats, const float *Ks,
    int32_t image_width, int32_t image_height, float eps2d, int32_t camera_model,
    const int32_t *radii, const float *rows, const float *grad_rows, const float *v_depths,
    const float *opacities /* [N]; needed when antialiased */, int32_t antialiased,
    float *v_means, float *v_covars, float *v_quats, float *v_scales, float *v_viewmats,
    float *v_opacities, float *v_colors,
    const float *v_means_add, /* [N,3] or NULL, as in gs_projection_bwd */
    const float *sh_coeffs, const float *sh_coeffs_rest, uint32_t sh_K, uint32_t sh_degree,
    float *v_sh_coeffs, float *v_sh_coeffs_rest,
    const float *sh_mask_logits, float sh_mask_temperature, int32_t sh_mask_binary, /* the forward's mask (or NULL, 0, 0) */
    float *v_sh_mask_logits /* [N] or NULL: gradient of the logits, every entry written (training-mode mask only) */,
    int32_t outputs_prefilled,
    gs_stream_t stream);

/* packed (COO) projection, replaces fully_fused_projection_packed_fwd_tensor
 *   (gsplat/cuda/csrc/fully_fused_projection_packed_fwd.cu:251-399).
 * Pass 1 (count): block_cnts[C * nblocks] <- #visible per (camera, 256-gaussian block),
 * nblocks = ceil(N / 256).  The caller turns it into an inclusive prefix sum
 * (gs_cumsum_i32) and reads nnz = last element.  Pass 2 (fill) writes rows in
 * (camera, gaussian) order.  NOTE the packed radius formula differs from the unpacked
 * one exactly as in the reference (packed_fwd.cu:183-186 vs fwd.cu:167-169). */
int32_t gs_projection_packed_count(
    uint32_t C, uint32_t N,
    const float *means, const float *covars, const float *quats, const float *scales,
    const float *viewmats, const float *Ks,
    int32_t image_width, int32_t image_height,
    float eps2d, float near_plane, float far_plane, float radius_clip,
    int32_t camera_model,
    int32_t *block_cnts, /* [C * ceil(N/256)] */
    gs_stream_t stream);

int32_t gs_projection_packed_fill(
    uint32_t C, uint32_t N,
    const float *means, const float *covars, const float *quats, const float *scales,
    const float *viewmats, const float *Ks,
    int32_t image_width, int32_t image_height,
    float eps2d, float near_plane, float far_plane, float radius_clip,
    int32_t camera_model,
    const int32_t *block_accum, /* inclusive prefix sum of block_cnts */
    int32_t *indptr,            /* [C+1] */
    int64_t *camera_ids,        /* [nnz] */
    int64_t *gaussian_ids,      /* [nnz] */
    int32_t *radii, float *means2d, float *depths, float *conics,
    float *compensations,       /* [nnz] or NULL */
    gs_stream_t stream);

/* replaces fully_fused_projection_packed_bwd_tensor
 *   (gsplat/cuda/csrc/fully_fused_projection_packed_bwd.cu:318-430).
 * sparse_grad == 0: dense [N,*] outputs, ACCUMULATED with atomics (caller zero-fills);
 * sparse_grad != 0: [nnz,*] outputs written directly. */
int32_t gs_projection_packed_bwd(
    uint32_t C, uint32_t N, uint32_t nnz,
    const float *means, const float *covars, const float *quats, const float *scales,
    const float *viewmats, const float *Ks,
    int32_t image_width, int32_t image_height, float eps2d, int32_t camera_model,
    const int64_t *camera_ids, const int64_t *gaussian_ids,
    const float *conics, const float *compensations,
    const float *v_means2d, const float *v_depths, const float *v_conics,
    const float *v_compensations,
    int32_t sparse_grad,
    float *v_means, float *v_covars, float *v_quats, float *v_scales, float *v_viewmats,
    gs_stream_t stream);

/* ------------------------------------------------------------------------
 * R2  spherical harmonics
 * replaces compute_sh_fwd_tensor / compute_sh_bwd_tensor
 *   (gsplat/cuda/csrc/compute_sh_fwd.cu:40-72, compute_sh_bwd.cu:53-95,
 *    gsplat/cuda/include/spherical_harmonics.cuh:13-362)
 * Elements are laid out [C, N]; coeffs is [C,N,K,3] (coeffs_shared == 0) or
 * [N,K,3] broadcast over cameras (coeffs_shared != 0) -- the broadcast form avoids
 * the reference's [C,N,K,3] materialisation (gsplat/cuda/_wrapper.py:72).
 * masks: optional uint8 [C,N]; colours of masked-out elements are left untouched.
 * bwd: v_coeffs is fully OVERWRITTEN (zeros for masked / inactive bases),
 * shape [N,K,3] when coeffs_shared (sum over cameras done in-kernel) else [C,N,K,3].
 * v_dirs (optional, [C,N,3]) is fully overwritten.
 * ---------------------------------------------------------------------- */
int32_t gs_sh_fwd(
    uint32_t C, uint32_t N, uint32_t K, uint32_t degree,
    const float *dirs, const float *coeffs, int32_t coeffs_shared,
    const uint8_t *masks, float *colors, gs_stream_t stream);

int32_t gs_sh_bwd(
    uint32_t C, uint32_t N, uint32_t K, uint32_t degree,
    const float *dirs, const float *coeffs, int32_t coeffs_shared,
    const uint8_t *masks, const float *v_colors,
    float *v_coeffs, float *v_dirs, gs_stream_t stream);

/* Fused "view" form used by rasterization() for coefficients shared by all cameras: the torch
 * ops around the reference's spherical_harmonics call (gsplat/rendering.py:372-392) are folded in:
 *   dirs = means[n] - campos[c]   (campos = inverse(viewmats)[:, :3, 3], [C,3]; with campos_from_viewmats != 0 the
 *                                  pointer holds the [C,4,4] world->camera matrices and the centre is derived in-kernel)
 *   mask = radii[c,n] > 0         (radii may be NULL: no mask)
 *   colors = max(SH + 0.5, 0)
 * bwd: colors_out is the forward output (gradient of the clamp); v_colors may be a strided view
 * (row stride v_colors_stride floats, e.g. 16 for the packed compositing gradient rows);
 * v_coeffs [N,K,3] and v_means [N,3] (= sum over cameras of d/d dirs; may be NULL) are OVERWRITTEN.
 * Optional riders (both NULL to disable): fwd writes opacities_cn[c,n] = opacities[n] for EVERY element (the
 * `opacities.repeat(C, 1)` of rendering.py:331); bwd writes v_opacities[n] = sum_c v_opacities_cn[c,n] (row stride
 * v_opacities_stride floats) -- the two extra torch kernels of the pipeline disappear into passes that run anyway.
 * bwd, outputs_prefilled != 0: the caller guarantees v_coeffs (and v_coeffs_rest) already hold zeros; the rows of
 * gaussians no camera sees are then not written (137 of the 193 MB at BASELINE config 2), and v_means is only DEFINED
 * for gaussians some camera sees. */
/* campos[c] = inverse(viewmats[c])[:3, 3] for affine world->camera matrices, closed form
 * (replaces torch.inverse(viewmats) of gsplat/rendering.py:370, which host-synchronises on ROCm). */
int32_t gs_camera_centers(uint32_t C, const float *viewmats, float *campos, gs_stream_t stream);
int32_t gs_sh_view_fwd(
    uint32_t C, uint32_t N, uint32_t K, uint32_t degree,
    const float *means, const float *campos, int32_t campos_from_viewmats, const float *coeffs,
    const float *coeffs_rest /* NULL, or SPLIT rows: coeffs is the DC band [N,1,3] and this the higher bands [N,K-1,3] -- the
                                trainer's sh0 / shN parameters taken as they are, without the torch.cat of
                                examples/simple_trainer.py:779-786 (193 MB each way at 1 M splats) */,
    const int32_t *radii,
    float *colors, uint32_t colors_stride /* row stride in floats: 3, or GS_ROW_FLOATS when `colors` is column GS_ROW_COLOR of the splat rows */,
    const float *opacities /* [N] or NULL */, float *opacities_cn /* [C,N] or NULL */, gs_stream_t stream);
int32_t gs_sh_view_bwd(
    uint32_t C, uint32_t N, uint32_t K, uint32_t degree,
    const float *means, const float *campos, int32_t campos_from_viewmats, const float *coeffs, const float *coeffs_rest,
    const int32_t *radii,
    const float *colors_out, uint32_t colors_out_stride, const float *v_colors, uint32_t v_colors_stride,
    float *v_coeffs, float *v_coeffs_rest /* [N,K-1,3] with coeffs_rest, else NULL */, float *v_means,
    const float *v_opacities_cn /* or NULL */, uint32_t v_opacities_stride, float *v_opacities /* [N] or NULL */,
    int32_t outputs_prefilled,
    gs_stream_t stream);

/* ------------------------------------------------------------------------
 * R3 / R4  tile intersection, 64-bit radix sort, offset encode
 * replaces isect_tiles_tensor / isect_offset_encode_tensor
 *   (gsplat/cuda/csrc/isect_tiles.cu:106-306, 356-389)
 * Protocol: gs_isect_count -> gs_cumsum_i32 (inclusive, int64 out; last element
 * = n_isects) -> caller allocates -> gs_isect_emit -> gs_sort_pairs_u64_i32 ->
 * gs_isect_offset_encode.
 * ---------------------------------------------------------------------- */
int32_t gs_isect_count(
    uint32_t n_elems,           /* C*N or nnz */
    const float *means2d, uint32_t means2d_stride /* row stride in floats: 2, or GS_ROW_FLOATS for the splat rows */,
    const int32_t *radii,
    uint32_t tile_size, uint32_t tile_width, uint32_t tile_height,
    int32_t *tiles_per_gauss,   /* [n_elems] */
    gs_stream_t stream);

/* inclusive prefix sum int32 -> int64.  scratch: gs_cumsum_scratch_bytes(n). */
size_t gs_cumsum_scratch_bytes(uint64_t n);
int32_t gs_cumsum_i32(
    uint64_t n, const int32_t *in, int64_t *out,
    void *scratch, size_t scratch_bytes, gs_stream_t stream);
/* int32 -> int32 variant (packed projection block counts). */
int32_t gs_cumsum_i32_i32(
    uint64_t n, const int32_t *in, int32_t *out,
    void *scratch, size_t scratch_bytes, gs_stream_t stream);

/* Splat-level depth pre-sort (an optimisation of the sorted path, results identical):
 * keys[i] = float_bits(depth_i) << 32 | i for visible elements, a maximal key for culled ones.
 * Sorting them (gs_sort_pairs_u64_i32, bits [32,64)) gives a permutation `perm` in (depth, index)
 * order; emitting the intersections in that order (gs_isect_emit with perm, cum_tiles being the
 * prefix sum of gs_gather_i32(tiles_per_gauss, perm)) leaves only the (camera, tile) bits
 * [32, 32+tile_bits+cam_bits) to be sorted afterwards -- 2 radix passes over the n_isects pairs
 * instead of 6 -- and, the radix sort being stable, yields exactly the order of a full-key sort
 * of the reference's emission order (ties: ascending flatten id). */
int32_t gs_isect_depth_keys(
    uint32_t n_elems, const int32_t *radii, const float *depths,
    int64_t *keys, int32_t *vals, gs_stream_t stream);
int32_t gs_gather_i32(uint32_t n, const int32_t *src, const int32_t *idx, int32_t *out, gs_stream_t stream);
/* the same in fewer launches: gs_isect_count + gs_isect_depth_keys in one kernel, and the inclusive prefix sum
 * of in[idx[i]] (= gs_gather_i32 followed by gs_cumsum_i32) without the intermediate array */
int32_t gs_isect_count_keys(
    uint32_t n_elems, const float *means2d /* NULL: tiles_per_gauss is an INPUT (gs_projection_rows_fwd counted) */, uint32_t means2d_stride, const int32_t *radii, const float *depths,
    uint32_t tile_size, uint32_t tile_width, uint32_t tile_height,
    int32_t *tiles_per_gauss, int64_t *keys, int32_t *vals /* element indices; may be NULL with bucket_splitters (the bucketed
                           pre-sort takes the element from the key's low half) */,
    int32_t *block_sums /* [gs_isect_count_blocks(n_elems)][2] (8-byte aligned) or NULL: per block (intersections, visible
                           elements), ONE 8-byte store; the totals are n_isects -- known here, before the depth pre-sort and the
                           prefix sum, so the host read-back of isect_tiles.cu:200 can overlap them -- and the number of
                           elements the pre-sort keeps (gs_isect_finish_presorted's n_kept_host) */,
    void *sort_temp, size_t sort_temp_bytes /* NULL, 0 -- or the temp buffer the keys will be sorted with
                           (gs_sort_pairs_u64_i32_drop over bits [32, 64)), when gs_sort_first_hist_applicable(n_elems): this
                           kernel then also counts the digits of that sort's first pass (pass first_hist_ready = 1 there) */,
    const int64_t *bucket_splitters /* NULL, or the table of gs_presort_split (with sort_temp = the temp buffer of
                           gs_presort_buckets): the histogram is then counted per BUCKET, for the bucketed pre-sort below */,
    gs_stream_t stream);
uint32_t gs_isect_count_blocks(uint32_t n_elems);
int32_t gs_cumsum_gather_i32(
    uint64_t n, const int32_t *in, const int32_t *idx, const uint32_t *n_valid /* device scalar or NULL: only out[0, *n_valid) is defined (hand the same n_valid to gs_isect_emit*) */,
    int64_t *out, void *scratch, size_t scratch_bytes, gs_stream_t stream);

int32_t gs_isect_emit(
    uint32_t n_elems, uint32_t N,   /* camera of element i = i / N when camera_ids NULL */
    const int32_t *perm,            /* [n_elems] emission order or NULL (identity) */
    const uint32_t *n_valid,        /* device scalar or NULL: only perm[0 .. *n_valid) is defined (gs_sort_pairs_u64_i32_drop) */
    const int64_t *camera_ids,      /* [nnz] or NULL */
    const float *means2d, uint32_t means2d_stride, const int32_t *radii, const float *depths,
    const int64_t *cum_tiles_per_gauss, /* inclusive, indexed by emission position */
    uint32_t tile_size, uint32_t tile_width, uint32_t tile_height,
    uint32_t tile_n_bits,
    int64_t *isect_ids,   /* [n_isects] */
    int32_t *flatten_ids, /* [n_isects] */
    gs_stream_t stream);

/* The sorted path in compact form (what rasterization() uses): gs_isect_emit_compact writes every (tile, splat) pair as a
 * 32-bit key  camera << tile_n_bits | tile  plus the flatten id (8 bytes instead of 12), in the depth order of `perm`;
 * gs_sort_isect_pairs sorts the pairs stably by the low `key_bits` (= tile_n_bits + cam_n_bits) bits of the key and its
 * LAST pass writes the reference's outputs: isect_ids = key << 32 | float_bits(depths[flatten id]) and flatten_ids --
 * bit-identical to gs_isect_emit + gs_sort_pairs_u64_i32 (isect_tiles.cu:89-103, 245-299).  keys32 / vals are scratch:
 * destroyed.  temp: gs_sort_isect_temp_bytes(n). */
int32_t gs_isect_emit_compact(
    uint32_t n_elems, uint32_t N, const int32_t *perm, const uint32_t *n_valid, const int64_t *camera_ids,
    const float *means2d, uint32_t means2d_stride, const int32_t *radii, const float *depths, const int64_t *cum_tiles_per_gauss,
    uint32_t tile_size, uint32_t tile_width, uint32_t tile_height, uint32_t tile_n_bits,
    uint32_t *keys32,     /* [n_isects] */
    int32_t *flatten_ids, /* [n_isects] */
    gs_stream_t stream);
/* The same emission with the prefix scan folded in, for the depth-pre-sorted path (perm from gs_sort_pairs_u64_i32_drop):
 * instead of cum_tiles_per_gauss it takes tiles_per_gauss (indexed by element) and group_sums[g] = the tiles of the emission
 * positions [g << s, (g + 1) << s), s = gs_isect_emit_group_shift() -- what that sort's last pass leaves behind in its
 * side_sums (side_vals = tiles_per_gauss, side_shift = s).  compact != 0: keys32 as gs_isect_emit_compact; else isect_ids. */
uint32_t gs_isect_emit_group_shift(void);
uint32_t gs_isect_emit_prefix_from_groups(void); /* more groups than this: hand group_prefix (gs_cumsum_i32 of group_sums) */
int32_t gs_isect_emit_presorted(
    uint32_t n_elems, uint32_t N, const int32_t *perm, const uint32_t *n_valid, const int64_t *camera_ids,
    const float *means2d, uint32_t means2d_stride, const int32_t *radii, const float *depths,
    const int32_t *tiles_per_gauss, const uint32_t *group_sums,
    const int64_t *group_prefix /* NULL, or the inclusive prefix sum of group_sums (gs_cumsum_i32): every workgroup adds up
                                   its predecessors' sums itself otherwise -- fine up to a few thousand groups */,
    uint32_t tile_size, uint32_t tile_width, uint32_t tile_height, uint32_t tile_n_bits, int32_t compact,
    int64_t *isect_ids, uint32_t *keys32, int32_t *flatten_ids, gs_stream_t stream);
/* The whole second half of the sorted binning in ONE call (what rasterization() issues right after its host read-back of
 * n_isects, while the GPU still works off the depth pre-sort: three entry points' worth of host work in one):
 * gs_isect_emit_presorted(compact) -> gs_sort_isect_pairs -> gs_isect_offset_encode.  work: caller-allocated,
 * gs_isect_finish_work_bytes(n_isects) bytes, 16-byte aligned (the compact pairs and the sort's temporaries).
 * gs_isect_finish_work_bytes is non-decreasing in n: a buffer sized for n serves every smaller count (callers allocate it for a
 * capacity before they know the count). */
size_t gs_isect_finish_work_bytes(uint64_t n_isects);
int32_t gs_isect_finish_presorted(
    uint32_t n_elems, uint32_t N, uint64_t n_isects, const int32_t *perm, const uint32_t *n_valid, const int64_t *camera_ids,
    const float *means2d, uint32_t means2d_stride, const int32_t *radii, const float *depths,
    const int32_t *tiles_per_gauss, const uint32_t *group_sums, const int64_t *group_prefix,
    uint32_t tile_size, uint32_t tile_width, uint32_t tile_height, uint32_t tile_n_bits, uint32_t cam_n_bits, uint32_t C,
    int64_t *isect_ids /* [n_isects] */, int32_t *flatten_ids /* [n_isects] */, int32_t *offsets /* [C, tile_height, tile_width] */,
    void *work, size_t work_bytes,
    uint32_t n_kept_host /* 0, or the number of elements in perm (*n_valid) when the host knows it (the block sums of
                            gs_projection_rows_fwd / gs_isect_count_keys): when (camera, tile) key and emission position fit 32
                            bits together the pairs then travel PACKED -- gs_isect_emit_packed + gs_sort_isect_packed, 4 bytes
                            per pair instead of 8 through emission and sort; same outputs */,
    const int64_t *sorted_keys /* NULL, or the pre-sort's sorted keys (depth bits << 32 | element, in perm's order: keys_out of
                            gs_sort_pairs_u64_i32_drop, keys_in of gs_presort_buckets after the call): the packed route's last pass
                            then fetches flatten id and depth bits with one gather */,
    gs_stream_t stream);
/* Row binning: the third route of gs_isect_finish_presorted.  The pairs of one splat are a rectangle of tiles and the splats
 * arrive in depth order, so nothing has to be sorted pair by pair: the (splat, tile row) entries -- a quarter of the pairs on a
 * 1080p frame -- are put into row order by ONE counting pass (row histogram per block of positions, scan, scatter of 8-byte
 * entries position | x0 | x1), and every row list is then expanded into its columns (column histogram per chunk of a row
 * list, scan, expand), which writes each output pair exactly once and yields the tile offsets from its own counts: six launches,
 * no pair array, no offsets launch.  Ranks depend on list order alone (lane masks per wave, wave order inside a block, block
 * order from the scans); same three outputs, bit for bit.  Taken when the packed route's preconditions hold (perm, n_kept_host
 * > 0, no camera_ids), tile_width <= GS_ROW_BINNING_MAX_WIDTH and C * tile_height <= GS_ROW_BINNING_MAX_ROWS (the counters of a
 * block live in LDS, one thread per column / row), C * tile_height * ceil(n_kept_host / 512) <= GS_ROW_BINNING_MAX_COUNTERS
 * (row counters per block of 512 positions: they stay a small fraction of the entries), n_isects < 2^31, at most 31 key bits in use, and
 * gs_isect_row_binning_work_bytes(...) fits the work buffer that was handed in (8 bytes per pair and per kept splat plus the
 * counters, against the 16 bytes per pair of gs_isect_finish_work_bytes, which is unchanged: it fits when the kept splats
 * cover two tiles or more on average); every other call takes the packed or the pair route as before.
 *   gs_isect_row_binning(on): process-wide switch; on = 0 / 1 sets it, a negative value only reads; returns the previous state.
 *   gs_isect_last_route(): GS_ISECT_ROUTE_* of the last gs_isect_finish_presorted call of this process that had pairs to bin. */
enum {
    GS_ROW_BINNING_MAX_WIDTH = 256,
    GS_ROW_BINNING_MAX_ROWS = 256,
    GS_ROW_BINNING_MAX_COUNTERS = 131072
};
enum { GS_ISECT_ROUTE_NONE = 0, GS_ISECT_ROUTE_PAIRS = 1, GS_ISECT_ROUTE_PACKED = 2, GS_ISECT_ROUTE_ROWS = 3 };
int32_t gs_isect_row_binning(int32_t on);
int32_t gs_isect_last_route(void);
size_t gs_isect_row_binning_work_bytes(uint64_t n_isects, uint32_t n_kept, uint32_t rows, uint32_t tile_width);
/* Packed pairs.  A pair is ONE 32-bit word  (camera << tile_n_bits | tile) << pos_bits | emission position, the position being
 * the splat's index in perm = its depth rank: the words of one tile are in depth order when the array is sorted stably on the
 * key bits, so no value array rides along, and the last pass writes the reference's outputs through perm:
 * flatten_ids = perm[position], isect_ids = key << 32 | float_bits(depths[flatten id]).  Needs key_bits (the bits a key can
 * have set, <= 31) + pos_bits (2^pos_bits >= number of elements in perm) <= 32.  words: scratch, destroyed.
 * temp: gs_sort_isect_temp_bytes(n). */
int32_t gs_isect_emit_packed(
    uint32_t n_elems, uint32_t N, const int32_t *perm, const uint32_t *n_valid, const int64_t *camera_ids,
    const float *means2d, uint32_t means2d_stride, const int32_t *radii, const float *depths,
    const int32_t *tiles_per_gauss, const uint32_t *group_sums, const int64_t *group_prefix,
    uint32_t tile_size, uint32_t tile_width, uint32_t tile_height, uint32_t tile_n_bits, uint32_t pos_bits,
    uint32_t *words /* [n_isects] */, gs_stream_t stream);
int32_t gs_sort_isect_packed(
    uint64_t n, uint32_t *words, const int32_t *perm, const int64_t *sorted_keys /* NULL, or (depth bits << 32 | element) by
    position: replaces perm + depths */, const float *depths /* indexed by the flatten id */, int32_t key_bits,
    uint32_t pos_bits, int64_t *isect_ids, int32_t *flatten_ids, void *temp, size_t temp_bytes, gs_stream_t stream);
/* non-decreasing in n: a buffer sized for n serves every smaller count (the sort's blocks are 1024 keys up to 2^21 keys and 4096
 * above; the block histogram is reserved for the larger of the two layouts there) */
size_t gs_sort_isect_temp_bytes(uint64_t n);
int32_t gs_sort_isect_pairs(
    uint64_t n, uint32_t *keys32, int32_t *vals, const float *depths /* indexed by the flatten id */, int32_t key_bits,
    int64_t *isect_ids, int32_t *flatten_ids, void *temp, size_t temp_bytes, gs_stream_t stream);

/* Stable LSD radix sort of (uint64 key, int32 value) pairs on key bits
 * [begin_bit, end_bit) -- the replacement for cub::DeviceRadixSort::SortPairs
 * (gsplat/cuda/csrc/isect_tiles.cu:245-299).  Inputs are not modified; the sorted
 * result is in keys_out / vals_out.
 * gs_sort_temp_bytes is non-decreasing in n: a buffer sized for n serves every smaller count. */
size_t gs_sort_temp_bytes(uint64_t n);
int32_t gs_sort_pairs_u64_i32(
    uint64_t n,
    const int64_t *keys_in, const int32_t *vals_in,
    int64_t *keys_out, int32_t *vals_out,
    int32_t begin_bit, int32_t end_bit,
    void *temp, size_t temp_bytes, gs_stream_t stream);
/* Same sort, but keys whose upper 32 bits equal drop_hi32 are DROPPED by the first pass (not counted, not written):
 * the outputs hold the *n_kept surviving pairs in sorted order (n_kept: device scalar, written by the call), the rest
 * of the output arrays is untouched.  Used for the splat-level depth pre-sort, where culled splats carry the maximal
 * key and would otherwise be moved through every pass (71% of the elements at BASELINE config 2). */
int32_t gs_sort_pairs_u64_i32_drop(
    uint64_t n, const int64_t *keys_in, const int32_t *vals_in, int64_t *keys_out, int32_t *vals_out,
    int32_t begin_bit, int32_t end_bit, uint32_t drop_hi32, uint32_t *n_kept,
    void *temp, size_t temp_bytes,
    int32_t first_hist_ready /* != 0: the first pass's block histogram is already in temp (gs_isect_count_keys) */,
    const int32_t *side_vals, uint32_t *side_sums, uint32_t side_shift /* both NULL, or: the LAST pass also leaves
                             side_sums[g] = sum of side_vals[vals_out[p]] over the output positions p in [g << side_shift,
                             (g + 1) << side_shift), for all ceil(n / 2^side_shift) groups -- the block sums of the prefix scan
                             gs_isect_emit_presorted needs (side_vals = tiles_per_gauss), with no launch of their own */,
    gs_stream_t stream);
int32_t gs_sort_first_hist_applicable(uint64_t n);

/* Bucketed depth pre-sort (round 4): the same result as gs_sort_pairs_u64_i32_drop over bits [32, 64) with drop_hi32 =
 * 0x7fffffff on the keys of gs_isect_count_keys -- perm = the elements in (depth bits, element) order, culled ones dropped --
 * in 4 launches instead of 11 for the sizes where every radix launch sits at its latency floor (gs_presort_applicable(n):
 * n <= 2 M elements):
 *   gs_presort_split     255 splitters at equal ranks among the visible ones of 8192 elements sampled at a regular stride
 *                        (round 6: individual elements fetched by 8 workgroups instead of 512 runs of 16 by one -- a spatially
 *                        sorted splat array made the runs' depths nearly equal and the buckets overflow).  splitters: int64
 *                        [gs_presort_split_elems()]: the 256-entry table in front, the call's candidate slots behind it (no
 *                        initialisation needed; two launches: 32 sampling workgroups, then the splitter workgroup)
 *   gs_isect_count_keys  (bucket_splitters = the table, sort_temp = temp) counts every 1024-element block's keys per bucket
 *   gs_presort_buckets   scan + ONE stable partition pass by bucket + local sorts: workgroup w finishes the buckets starting in
 *                        positions [1024 w, 1024 (w + 1)) with an LSD sort in LDS on the depth bits that differ inside its range.
 * A range above lds_capacity keys (0 = gs_presort_capacity() = 4096; smaller values are for tests) is sorted by its workgroup
 * through global memory: slower, same result -- with sampled splitters that takes adversarial input.
 * temp: gs_presort_temp_bytes(n) -- non-decreasing in n: a buffer sized for n serves every smaller count.
 * side_vals / side_sums / side_shift: as in gs_sort_pairs_u64_i32_drop (side_sums is zeroed by the call). */
int32_t gs_presort_applicable(uint64_t n);
uint32_t gs_presort_capacity(void);
size_t gs_presort_temp_bytes(uint64_t n);
uint32_t gs_presort_split_elems(void);
int32_t gs_presort_split(
    uint32_t n_elems, const int32_t *radii, const float *depths, int64_t *splitters /* [gs_presort_split_elems()], see above */,
    gs_stream_t stream);
int32_t gs_presort_buckets(
    uint64_t n, int64_t *keys_in /* DESTROYED: on return [0, *n_kept) holds the sorted keys (depth bits << 32 | element), what
    gs_isect_finish_presorted takes as sorted_keys */, const int32_t *vals_in /* unused (may be NULL) */, const int64_t *splitters,
    int32_t *perm /* [n]; [0, *n_kept) written */, uint32_t *n_kept /* device scalar, written */,
    void *temp, size_t temp_bytes, const int32_t *side_vals, uint32_t *side_sums, uint32_t side_shift,
    uint32_t lds_capacity, gs_stream_t stream);

int32_t gs_isect_offset_encode(
    uint32_t n_isects, const int64_t *isect_ids_sorted,
    uint32_t C, uint32_t n_tiles, uint32_t tile_n_bits,
    int32_t *offsets, /* [C, n_tiles]; fully written (zeros when n_isects == 0) */
    gs_stream_t stream);

/* ------------------------------------------------------------------------
 * R5  per-tile alpha compositing
 * replaces rasterize_to_pixels_fwd_tensor / rasterize_to_pixels_bwd_tensor
 *   (gsplat/cuda/csrc/rasterize_to_pixels_fwd.cu:187-352, kernel 16-185;
 *    gsplat/cuda/csrc/rasterize_to_pixels_bwd.cu:279-489, kernel 17-277)
 * channels is a runtime value (1..513); no padding is required from the caller.
 * n_elems = C*N (unpacked) or nnz (packed): size of the per-splat arrays.
 * bwd outputs are ACCUMULATED with atomics: caller zero-fills them.
 * Channel counts: 1..4 and 5..16 run as one launch each way (tile forward + depth-segmented backward, colours in the LDS
 * records), 17..32 as two launches over halves of the channels (the gradients are linear in v_render_colors; with absgrad,
 * which is not, the backward of more than 16 channels takes the generic one-pass kernel), more than 32 the generic kernels.
 * scratch (optional, gs_raster_plan.scratch_bytes bytes): the forward stores per-pixel checkpoints (transmittance, accumulated colour) at fixed
 * list-index boundaries in it; when the SAME buffer (contents preserved) and the forward's
 * render_colors are handed to gs_rasterize_bwd, the backward runs depth-segmented (one wave per
 * (tile, segment), no serial walk of long lists).  Without them it falls back to one wave per
 * quadrant.  Results are the same up to fp32 rounding.
 * ---------------------------------------------------------------------- */
/* The launch plan of one gs_rasterize_fwd / gs_rasterize_bwd pair: a HOST struct the caller owns, filled by
 * gs_rasterize_plan and handed to both calls, so the two cannot disagree about the scratch layout and the library
 * keeps no state of its own (no process-global tuning).  tuning: NULL (the measured MI355X optima) or 4 ints
 *   [0] segment length of the depth-segmented backward in list entries (multiple of 64; 0 = unsegmented; default 256)
 *   [1] list length from which a tile's four forward waves stop cooperating (0 = never; default 2048)
 *   [2] / [3] work items per XCD group of the forward / backward (0 = identity mapping; default 16)
 * a negative entry keeps the default.  Results never depend on the plan beyond floating-point association of the
 * gradient atomics.  scratch_bytes: size of the scratch buffer both calls take (forward checkpoints, the backward's
 * work list).  Unlike the sort's size queries, scratch_bytes carries NO guarantee of being non-decreasing in n_isects
 * (the segment length doubles where the checkpoints would pass their bound, which halves them): callers size the scratch
 * exactly, from the plan of the very call, and the calls insist on that plan. */
typedef struct gs_raster_plan {
    uint32_t magic, n_tiles_all, n_isects, channels;
    int32_t seg, solo_min;
    uint32_t xcd_fwd, xcd_bwd;
    uint64_t scratch_bytes;
    uint32_t reserved[6];
} gs_raster_plan;
int32_t gs_rasterize_plan(uint32_t n_tiles_all /* C * tile_width * tile_height */, uint32_t n_isects, uint32_t channels,
                          const int32_t *tuning /* [5] HOST ints or NULL */, gs_raster_plan *plan);

int32_t gs_rasterize_fwd(
    uint32_t C, uint32_t n_elems, uint32_t n_isects, uint32_t channels,
    const float *means2d, const float *conics, const float *colors,
    const float *opacities,
    const uint32_t *splat_strides, /* NULL: the reference's dense arrays (rows of 2 / 3 / channels / 1 floats); else 4 HOST
                                      ints: row strides in floats of means2d, conics, colors, opacities.  When all four
                                      are GS_ROW_FLOATS and the pointers are columns 0 / 2 / 6 / 5 of one 64-byte-aligned
                                      row buffer (channels <= 4), the kernels fetch whole splat rows; with more than 4
                                      channels the same holds for the geometry alone (means2d / conics / opacities at
                                      columns 0 / 2 / 5 with stride GS_ROW_FLOATS, colours in their own array) */
    const float *backgrounds, /* [C,channels] or NULL */
    const uint8_t *masks,     /* [C,tile_h,tile_w] or NULL */
    uint32_t image_width, uint32_t image_height, uint32_t tile_size,
    uint32_t tile_width, uint32_t tile_height,
    const int32_t *tile_offsets, const int32_t *flatten_ids,
    float *render_colors, /* [C,H,W,channels] */
    float *render_alphas, /* [C,H,W,1] */
    int32_t *last_ids,    /* [C,H,W] */
    const gs_raster_plan *plan, void *scratch, /* both NULL: no checkpoints (inference, or an unsegmented backward) */
    void *zero_fill, size_t zero_fill_bytes, /* optional side job (NULL, 0: none): a 16-byte aligned buffer this call
                                                zero-fills, its stores spread over the tile workgroups' last instructions --
                                                meant for the gradient rows the matching gs_rasterize_bwd accumulates into,
                                                which then need no fill pass of their own */
    gs_stream_t stream);

int32_t gs_rasterize_bwd(
    uint32_t C, uint32_t n_elems, uint32_t n_isects, uint32_t channels,
    const float *means2d, const float *conics, const float *colors,
    const float *opacities, const uint32_t *splat_strides /* as in gs_rasterize_fwd */,
    const float *backgrounds, const uint8_t *masks,
    uint32_t image_width, uint32_t image_height, uint32_t tile_size,
    uint32_t tile_width, uint32_t tile_height,
    const int32_t *tile_offsets, const int32_t *flatten_ids,
    const float *render_colors, /* forward output, or NULL (disables the segmented path) */
    const float *render_alphas, const int32_t *last_ids,
    const float *v_render_colors, const float *v_render_alphas /* or NULL (= zero) */,
    int64_t v_render_colors_pixel_stride,   /* element strides of v_render_colors: (channels, 1) for a dense */
    int64_t v_render_colors_channel_stride, /* [C,H,W,channels] tensor; (0, 0) for a broadcast scalar (the gradient
                                               of sum(render)): nothing has to be materialised */
    float *v_means2d_abs, /* [n_elems,2] or NULL */
    float *v_means2d,     /* [n_elems,2] */
    float *v_conics,      /* [n_elems,3] */
    float *v_colors,      /* [n_elems,channels] */
    float *v_opacities,   /* [n_elems] */
    int32_t packed16,     /* != 0: v_means2d is ONE zero-filled [n_elems,16] buffer receiving every gradient (the splat-row
                             columns, see above); v_conics / v_colors / v_opacities are ignored, v_means2d_abs only
                             selects absgrad (non-NULL).  One 64-byte row per splat lets the kernels add a whole splat's
                             gradient with a single L2 request.  1 requires channels <= 4.
                             2 (more than 4 channels): the GEOMETRY rows only -- v_means2d is the zero-filled [n_elems,16]
                             buffer (columns 0..5 and, with absgrad, 10 / 11), the colour gradients go to v_colors
                             [n_elems,channels] (zero-filled by the caller): the form the 5..32-channel kernels want,
                             and gs_projection_rows_bwd reads the rows in place */
    int64_t *det_accum,   /* NULL, or DETERMINISTIC mode (channels <= 4): a zero-filled int64 [n_elems,2,12] buffer.  The per-splat
                             sums are then accumulated in fixed point with integer atomics (the order in which the work
                             items reach a splat no longer matters; two accumulators per value: units of 2^-38 for
                             contributions below 2^10, of 2^-6 above) and converted into the float outputs by a second
                             kernel, which OVERWRITES every row of them: two runs give bit-identical gradients.  The
                             reference's float atomics are not reproducible either (rasterize_to_pixels_bwd.cu:243-274). */
    const gs_raster_plan *plan, void *scratch, /* the forward's plan and scratch (contents preserved), or NULL, NULL */
    gs_stream_t stream);

/* ------------------------------------------------------------------------
 * Q1 / Q2  per-splat quantize / dequantize straight-through estimators
 * replaces the torch ops of fake_quantize_ste / STE
 *   (gsplat/compression_simulation/ops.py:39-54, 57-75)
 * noise: out = clamp(x, lo, hi) + noise * q_step   (noise supplied by the caller so the
 *        RNG stream stays torch's), bwd: v_x = v_out where lo <= x <= hi else 0.
 * round: x <- clamp(x, lo, hi) IN PLACE (the reference mutates the parameter),
 *        out = round_half_even(((x - lo) / (hi - lo)) / q) * q * (hi - lo) + lo,
 *        q = 1/(2^bits - 1); bwd is the identity (no kernel).
 * All arithmetic is IEEE fp32 with no contraction, in the reference's op order.
 * activation (opt-in fusion, GS_ACT_*): out = act(quantized value) -- the torch.exp / torch.sigmoid the trainer applies to
 * the hooked log-scales / opacity logits (examples/simple_trainer.py:779-786) in the same pass; the backward multiplies by
 * act' (read off `out`, the forward's output).  GS_ACT_NONE is the reference's bit-exact path.
 * ---------------------------------------------------------------------- */
int32_t gs_quantize_noise_fwd(
    uint64_t n, const float *x, const float *noise,
    float lo, float hi, float q_step, int32_t activation, float *out, gs_stream_t stream);
int32_t gs_quantize_noise_bwd(
    uint64_t n, const float *x, const float *v_out,
    float lo, float hi, int32_t activation, const float *out /* forward output; NULL with GS_ACT_NONE */,
    float *v_x, gs_stream_t stream);
int32_t gs_quantize_round_fwd(
    uint64_t n, float *x_inplace, float lo, float hi, float range /* (float)(hi-lo) */,
    float q_step_norm /* (float)(1/(2^bits-1)) */, int32_t activation, float *out, gs_stream_t stream);
/* round mode with a fused activation: v_x = v_out * act'(out) for every element (without an activation the gradient is the
 * identity and there is nothing to launch) */
int32_t gs_quantize_round_bwd(
    uint64_t n, const float *v_out, int32_t activation, const float *out, float *v_x, gs_stream_t stream);

/* Multi-tensor "noise" quantizer with the noise generated in the kernel (the hooks of BASELINE config 3 in ONE launch each way;
 * the noise never exists in memory).  Bit-identical to  noise = torch.empty_like(x).uniform_(-0.5, 0.5)  followed by
 * gs_quantize_noise_fwd, tensor after tensor: the kernel evaluates the Philox4x32-10 draws torch's uniform_ kernel would have
 * made for (philox_seed, philox_offset) -- see csrc/quantize.hip for the counter scheme.  The caller reads seed and offset from
 * the device's default generator and advances it by gs_quantize_philox_advance(n, grid_cap) per tensor, so the process's RNG
 * stream is exactly the reference's.  grid_cap = CUs * (max threads per CU / 256) of the device (what torch caps uniform_'s grid
 * at).  descs: HOST array (copied into the kernel arguments). */
#define GS_QUANT_MULTI_MAX 8
typedef struct gs_quant_desc {
    uint64_t n;             /* floats in the tensor (0: skipped) */
    const float *x;         /* input */
    float *out;             /* fwd: output; bwd: the forward's output (only read with an activation) */
    const float *v_out;     /* bwd: upstream gradient */
    float *v_x;             /* bwd: gradient out */
    float lo, hi, q_step;
    int32_t activation;     /* GS_ACT_* fused behind the quantizer */
    uint64_t philox_offset; /* fwd: the generator's offset when this tensor's uniform_ call would have run (multiple of 4) */
} gs_quant_desc;
uint64_t gs_quantize_philox_advance(uint64_t n, uint32_t grid_cap);
int32_t gs_quantize_noise_multi_fwd(
    uint32_t n_tensors, const gs_quant_desc *descs, uint64_t philox_seed, uint32_t grid_cap, gs_stream_t stream);
int32_t gs_quantize_noise_multi_bwd(uint32_t n_tensors, const gs_quant_desc *descs, gs_stream_t stream);
/* The round mode for several tensors in one launch each way (round 6): gs_quantize_round_fwd's arithmetic per element.  descs[t].x is
 * the parameter and descs[t].v_x its WRITABLE alias (the same pointer: the parameter is clamped in place, ops.py:63), out the grid
 * value (activated when descs[t].activation is set); ranges[t] = hi - lo and q_step_norms[t] = 1 / (2^bits - 1), both computed as the
 * reference does (python double, then float); HOST arrays.  The backward is the identity (no call needed) except behind a fused
 * activation: gs_quantize_round_multi_bwd writes v_x = v_out x d act (out), no clamp mask, for the descriptors with n > 0. */
int32_t gs_quantize_round_multi_fwd(uint32_t n_tensors, const gs_quant_desc *descs, const float *ranges, const float *q_step_norms,
                                    gs_stream_t stream);
int32_t gs_quantize_round_multi_bwd(uint32_t n_tensors, const gs_quant_desc *descs, gs_stream_t stream);


/* ------------------------------------------------------------------------
 * Q3  learnable per-splat mask on the higher SH bands ("shN adaptive mask") of the compression-simulation hooks
 * replaces the torch ops of AnnealingMask (gsplat/compression_simulation/ada_mask.py:6-62), applied by
 * CompressionSimulation.simulate_compression_shN (simulation.py:319-324), and of the "gradient" strategy's
 * shN_gradient_threshold (simulation.py:327-348).
 *   x [n, row]: the shN parameter, row = 3 (K - 1) floats per splat (45 at SH degree 3); mask_logits [n].
 *   training (binary = 0): mask = sigmoid(logit / temperature); eval (binary = 1): mask = sigmoid(logit) >= 0.5 (ada_mask.py:39)
 *   fwd: out = x * mask.
 *   bwd: v_x = v_out * mask (NULL: not wanted); v_mask_logits[n] = (sum_j v_out[n,j] x[n,j]) * mask (1 - mask) / temperature
 *        (NULL: not wanted; must be NULL with binary = 1), every row written, reduced without atomics (deterministic).
 * IEEE fp32, no contraction, torch's operation order (true division by the temperature, sigmoid = 1 / (1 + exp(-v))).
 * ---------------------------------------------------------------------- */
int32_t gs_shn_mask_fwd(
    uint64_t n, uint32_t row, const float *x, const float *mask_logits, float temperature, int32_t binary,
    float *out, gs_stream_t stream);
int32_t gs_shn_mask_bwd(
    uint64_t n, uint32_t row, const float *x, const float *mask_logits, float temperature, int32_t binary,
    const float *v_out, float *v_x, float *v_mask_logits, gs_stream_t stream);
/* the mask itself, one float per splat (binary = 1: get_binary_mask, ada_mask.py:42-44) */
int32_t gs_mask_values(
    uint64_t n, const float *mask_logits, float temperature, int32_t binary, float *out, gs_stream_t stream);
/* out[0] = (sum_i mask_i) / divisor in fp32 -- the mean of the soft mask behind get_sparsity_loss (ada_mask.py:46-58:
 * divisor = n) or, with binary = 1, get_mask_ratio's count / shape[0] (ada_mask.py:60-62).  temp: gs_mask_sum_temp_bytes()
 * bytes of scratch; the sum is accumulated in double in a fixed order (deterministic). */
size_t gs_mask_sum_temp_bytes(void);
int32_t gs_mask_sum(
    uint64_t n, const float *mask_logits, float temperature, int32_t binary, float divisor, void *temp, float *out,
    gs_stream_t stream);
/* gradient of that mean (binary = 0): v_mask_logits[i] = (v_mean[0] / divisor) * (1 - y) y / temperature, y = sigmoid(logit_i / T) */
int32_t gs_mask_mean_bwd(
    uint64_t n, const float *mask_logits, float temperature, const float *v_mean /* device scalar */, float divisor,
    float *v_mask_logits, gs_stream_t stream);
/* "gradient" strategy (simulation.py:327-348), two launches, no host read-back: zero_rows[n] <- 1 where every value of x's
 * row is exactly 0, *n_zero <- their count; threshold = 2e-3 when 1 - n_zero / n < 0.10, else 100; the rows of grad_inplace
 * whose x row is all zero AND whose Frobenius norm is below the threshold are set to 0. */
int32_t gs_shn_grad_threshold(
    uint64_t n, uint32_t row, const float *x, float *grad_inplace, uint8_t *zero_rows /* [n] scratch / output */,
    uint64_t *n_zero /* device scalar, output */, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * Factorized-prior bits estimator (the rate term behind the quantize hooks).
 * Replaces Entropy_factorized_optimized_refactor.forward
 * (gsplat/compression_simulation/entropy_model.py:195-254) and the autograd graph torch builds from
 * it: bits[n,c] = -log2(max(bound, |sigmoid(s u) - sigmoid(s l)|)), l/u = f_p(x[n,c] -/+ half_q[c]),
 * f_p a 1 -> W -> .. -> W -> 1 MLP (hidden_layers x hidden_width; reference: filters=(3,3) or (3,3,3))
 * with softplus'd matrices and tanh-gated residual nonlinearity (229-238), s = -sign(l+u) (247),
 * LowerBound gradient rule (355-357).  The parameter set of element (n,c) follows the reference's
 * 32-way reshape: p = (32 c + n / chunk) % channels, chunk = (n_rows + 32 - n_rows % 32) / 32.
 * params [channels, P] raw (un-transformed) parameters, per set and per layer [matrix row-major |
 * bias | factor], the last layer without factor; P = gs_entropy_factorized_params_per_channel().
 * x, bits, v_bits, v_x: [n_rows, channels] row-major.  half_q: [channels] device floats (= Q/2).
 * bwd: v_x is overwritten; v_params [replicas, channels, P] is ACCUMULATED with atomics (zero-fill first)
 * and the caller sums it over the leading axis -- workgroups spread over the replicas because
 * same-address device-scope float atomics serialise (replicas = 1 is valid, 32 is what the wrapper uses).
 * hidden_layers, hidden_width in 1..4 (uniform width), channels in 1..32; anything else: status 1. */
uint32_t gs_entropy_factorized_params_per_channel(uint32_t hidden_layers, uint32_t hidden_width);
int32_t gs_entropy_factorized_fwd(
    uint64_t n_rows, uint32_t channels, uint32_t hidden_layers, uint32_t hidden_width,
    const float *x, const float *half_q, const float *params, float likelihood_bound,
    float *bits, gs_stream_t stream);
int32_t gs_entropy_factorized_bwd(
    uint64_t n_rows, uint32_t channels, uint32_t hidden_layers, uint32_t hidden_width,
    const float *x, const float *half_q, const float *params, float likelihood_bound,
    const float *v_bits, float *v_x, float *v_params, uint32_t replicas, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * Hash-grid Gaussian entropy model (the reference trainer's `--entropy_model_type gaussian_model`).
 * gs_hashgrid_encode_*: replaces the reference's CUDA-only `_gridencoder` extension (third_party/gridencoder/src/
 * gridencoder.cu kernel_grid / kernel_grid_backward / kernel_input_backward, driven by
 * gsplat/compression_simulation/gaussian_distribution_model.py:56-346), float32 only, for 1..4 grids in ONE launch:
 * grid g has its own raw table params[g] [rows[g], n_features], num_dim[g] in {2, 3}, an axis selector axes[g]
 * (which columns of pos are its coordinates: 0 = xyz, 1 = xy, 2 = xz, 3 = yz) and n_levels[g] levels whose resolutions / offsets
 * (n_levels[g] / n_levels[g] + 1 entries) follow each other in the two concatenated lists.  params, v_params, rows,
 * num_dim, axes, n_levels, resolutions and offsets are HOST arrays (params / v_params: host arrays of device pointers);
 * pos [n, pos_dim] (pos_dim 3, or 2 for a lone xy grid), out / v_out [n, sum(n_levels) * n_features] row-major in the
 * order of the grids and their levels (the reference's [L, N, F] buffer and its permute do not exist), v_pos [n, pos_dim].
 * Per (point, level), with R the resolution and T = offsets[l+1] - offsets[l]: a coordinate outside [0, 1] or NaN gives 0
 * outputs and no gradient (the reference lets NaN through); p = u * float(R - 2) + 0.5f in two float32 roundings,
 * g = floor(p), f = p - g; corner i has c[d] = g[d] or min(g[d] + 1, R - 1) (bit d of i) and weight prod(bit ? f : 1 - f); a
 * corner with any c[d] in {0, R - 1} takes no part; row = (dense index while the stride fits T, else xor of
 * c[d] * {1, 2654435761, 805459861}) % T, so every access is inside the level's slice; out = sum w / wn * E[row] with wn the
 * participating weights' sum (1e-9 if 0).  ste_binary != 0: E = (p >= 0) - (p < 0) of the raw parameter (STE_binary, 0
 * for NaN), and the table gradient passes where -1 <= p <= 1; ste_binary == 0: E = p.
 * bwd: v_params[g] is ACCUMULATED with float atomics (zero-fill first); v_pos is OVERWRITTEN with the reference's dy_dx
 * formula (finite differences of the corner values, a border corner counting as 0, wn not entering) summed over all grids
 * and levels by one owner per point -- no atomics, bit-identical from run to run.  v_params (or single entries of it) and
 * v_pos may be NULL: that gradient is skipped.  n_features in {1, 2, 4}, at most 32 levels in total, R in 3..2^24, offsets
 * ascending from >= 0 with offsets[last] <= rows, tables / out / v_out aligned to n_features floats; anything else:
 * status 1 and nothing is written.  n == 0 launches nothing.
 * gs_gaussian_bits_*: Entropy_gaussian.forward's likelihood (entropy_model.py:327-338) in one elementwise launch each
 * way.  x, bits, v_bits, v_x [n_rows, channels]; net, v_net [n_rows, 2 channels] = the regressor's output (means in columns
 * 0..C-1, raw scales in C..2C-1, read in place); half_q [channels] device floats (= Q/2).  s = max(scale, 1e-9),
 * like = |Phi((x + hq - m) / s) - Phi((x - hq - m) / s)| (erfc differences on the side where both are small: the tails keep
 * their relative accuracy), bits = -log2(max(bound, like)).  bwd OVERWRITES v_x and v_net: LowerBound rule (passes where
 * like >= bound or the likelihood's incoming gradient is negative), sign of the abs, clamp gate (scale >= 1e-9).
 * channels in 1..32; anything else, or a null pointer: status 1. */
int32_t gs_hashgrid_encode_fwd(
    uint64_t n, uint32_t pos_dim, uint32_t n_grids, uint32_t n_features, uint32_t ste_binary, const float *pos,
    const float *const *params, const uint64_t *rows, const uint32_t *num_dim, const uint32_t *axes,
    const uint32_t *n_levels, const int32_t *resolutions, const int32_t *offsets, float *out, gs_stream_t stream);
int32_t gs_hashgrid_encode_bwd(
    uint64_t n, uint32_t pos_dim, uint32_t n_grids, uint32_t n_features, uint32_t ste_binary, const float *pos,
    const float *const *params, const uint64_t *rows, const uint32_t *num_dim, const uint32_t *axes,
    const uint32_t *n_levels, const int32_t *resolutions, const int32_t *offsets, const float *v_out,
    float *const *v_params, float *v_pos, gs_stream_t stream);
int32_t gs_gaussian_bits_fwd(
    uint64_t n_rows, uint32_t channels, const float *x, const float *net, const float *half_q, float likelihood_bound,
    float *bits, gs_stream_t stream);
int32_t gs_gaussian_bits_bwd(
    uint64_t n_rows, uint32_t channels, const float *x, const float *net, const float *half_q, float likelihood_bound,
    const float *v_bits, float *v_x, float *v_net, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * Unfused public ops (reference: quat_scale_to_covar_preci_{fwd,bwd}.cu,
 * world_to_cam_{fwd,bwd}.cu, proj_{fwd,bwd}.cu)
 * ---------------------------------------------------------------------- */
int32_t gs_quat_scale_to_covar_preci_fwd(
    uint32_t N, const float *quats, const float *scales, int32_t triu,
    float *covars /* [N,3,3] or [N,6] or NULL */,
    float *precis /* same or NULL */, gs_stream_t stream);
int32_t gs_quat_scale_to_covar_preci_bwd(
    uint32_t N, const float *quats, const float *scales, int32_t triu,
    const float *v_covars, const float *v_precis, /* either may be NULL */
    float *v_quats, float *v_scales,              /* overwritten */
    gs_stream_t stream);

/* world_to_cam: means_c[c,n] = R_c p_n + t_c, covars_c[c,n] = R_c S_n R_c^T on GENERAL 3x3 matrices
 * (reference world_to_cam_fwd_tensor, csrc/world_to_cam_fwd.cu:85-127; device code
 * include/transform.cuh:8-46).  Either output (with its input) may be NULL.
 * bwd (world_to_cam_bwd_tensor, csrc/world_to_cam_bwd.cu:125-195; transform.cuh:19-68): v_means [N,3] and
 * v_covars [N,3,3] are OVERWRITTEN (summed over cameras inside the lane), v_viewmats [C,4,4] is
 * ACCUMULATED with atomics (zero-fill first); any of the three may be NULL (= not needed). */
int32_t gs_world_to_cam_fwd(
    uint32_t C, uint32_t N, const float *means /* [N,3] */, const float *covars /* [N,3,3] */,
    const float *viewmats /* [C,4,4] */, float *means_c /* [C,N,3] */, float *covars_c /* [C,N,3,3] */,
    gs_stream_t stream);
int32_t gs_world_to_cam_bwd(
    uint32_t C, uint32_t N, const float *means, const float *covars, const float *viewmats,
    const float *v_means_c /* [C,N,3] or NULL */, const float *v_covars_c /* [C,N,3,3] or NULL */,
    float *v_means, float *v_covars, float *v_viewmats, gs_stream_t stream);

/* proj: camera-space gaussians -> image plane, means2d [C,N,2], covars2d [C,N,2,2] = J S J^T with the
 * pinhole / orthographic / fisheye Jacobian (reference proj_fwd_tensor, csrc/proj_fwd.cu:81-129,
 * proj_bwd_tensor, csrc/proj_bwd.cu:128-182; device code include/proj.cuh).  No culling, general 3x3 S.
 * bwd overwrites v_means [C,N,3] and v_covars [C,N,3,3]. */
int32_t gs_proj_fwd(
    uint32_t C, uint32_t N, const float *means /* [C,N,3] */, const float *covars /* [C,N,3,3] */,
    const float *Ks /* [C,3,3] */, int32_t width, int32_t height, int32_t camera_model,
    float *means2d, float *covars2d, gs_stream_t stream);
int32_t gs_proj_bwd(
    uint32_t C, uint32_t N, const float *means, const float *covars, const float *Ks,
    int32_t width, int32_t height, int32_t camera_model,
    const float *v_means2d, const float *v_covars2d, float *v_means, float *v_covars, gs_stream_t stream);

/* rasterize_to_indices_in_range (reference rasterize_to_indices_in_range_tensor,
 * csrc/rasterize_to_indices_in_range.cu:177-300, kernel 16-175): for the list batches
 * [range_start, range_end) of every tile (one batch = tile_size^2 sorted entries) and the per-pixel
 * transmittances reached so far, list the (gaussian, pixel) pairs that get composited.
 * Two-call protocol: _count writes chunk_cnts i32 [C*H*W] (zero-fill first: untouched tiles stay 0), the
 * caller forms the exclusive prefix sum chunk_starts (i32, like the reference's int32 cumsum) and
 * the total, allocates, then _fill writes gaussian_ids (= flatten id % N) and pixel_ids
 * (= camera * H * W + row * W + column), both i64, pixel-major, list order inside a pixel. */
int32_t gs_rasterize_indices_count(
    uint32_t range_start, uint32_t range_end, uint32_t C, uint32_t N, uint32_t n_isects,
    const float *means2d, const float *conics, const float *opacities,
    uint32_t image_width, uint32_t image_height, uint32_t tile_size, uint32_t tile_width, uint32_t tile_height,
    const int32_t *tile_offsets, const int32_t *flatten_ids, const float *transmittances,
    int32_t *chunk_cnts, gs_stream_t stream);
int32_t gs_rasterize_indices_fill(
    uint32_t range_start, uint32_t range_end, uint32_t C, uint32_t N, uint32_t n_isects,
    const float *means2d, const float *conics, const float *opacities,
    uint32_t image_width, uint32_t image_height, uint32_t tile_size, uint32_t tile_width, uint32_t tile_height,
    const int32_t *tile_offsets, const int32_t *flatten_ids, const float *transmittances,
    const int32_t *chunk_starts, int64_t *gaussian_ids, int64_t *pixel_ids, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * On-disk attribute format: per-channel min-max quantization of a row-major
 * [rows, channels] grid and its exact inverse -- the arithmetic of _compress_png / _compress_png_kbit /
 * _compress_png_16bit and the matching _decompress_* (gsplat/compression/png_compression.py:166-389)
 * without the PNG container.  bits 1..8: ONE uint8 plane holding round(norm * (2^bits - 1)) << (8 - bits);
 * bits 16: low and high byte planes.  mins / maxs: [channels] device floats (torch.amin / amax of the grid).
 * Encode is fp32 with round-half-to-even, decode is float64 then cast, exactly like the numpy / torch mix
 * of the reference, so both are bit-exact against it. */
int32_t gs_grid_quantize(
    uint64_t n /* rows * channels */, uint32_t channels, const float *x, const float *mins, const float *maxs,
    uint32_t bits, uint8_t *plane_lo, uint8_t *plane_hi /* 16-bit only, else NULL */, gs_stream_t stream);
int32_t gs_grid_dequantize(
    uint64_t n, uint32_t channels, const uint8_t *plane_lo, const uint8_t *plane_hi /* or NULL */,
    const float *mins, const float *maxs, uint32_t bits, float *out, gs_stream_t stream);

/* Decode of the compressed attribute planes STRAIGHT INTO rasterization()'s inputs: replaces the
 * host-side chain of the reference's eval path -- PngCompression.decompress (gsplat/compression/png_compression.py:166-236:
 * _decompress_png_16bit for the means, _decompress_png_kbit / _decompress_png for scales, quats, opacities, sh0), the
 * inverse log transform of the means (228-230) and the trainer's activations (examples/simple_trainer.py:779-786) -- by one
 * kernel over the uint8 planes.  Planes are the [n, C] row-major views of the reference's [side, side, C] images; k-bit
 * planes keep their value in the top bits of the byte (as stored).  mins14 / maxs14 are HOST arrays: the per-channel
 * bounds of meta.json in the order means(3) scales(3) quats(4) opacities(1) sh0(3); bits5 (host): bit depth per attribute,
 * means = 16.  activate = 1: scales = exp(.), opacities = sigmoid(.) (what rasterization() takes); 0: the trainer's raw
 * parameters, bit-identical to gs_grid_dequantize.  normalize_quats = 1: quats / max(||quats||, 1e-12). */
int32_t gs_decode_splats(
    uint64_t n, const uint8_t *means_lo, const uint8_t *means_hi, const uint8_t *scales, const uint8_t *quats,
    const uint8_t *opacities, const uint8_t *sh0, const float *mins14, const float *maxs14, const uint32_t *bits5,
    int32_t normalize_quats, int32_t activate, float *means_out, float *scales_out, float *quats_out, float *opacities_out,
    float *sh0_out, gs_stream_t stream);
/* The inverse log transform of the means, out = sign(y) * expm1(|y|) (gsplat/utils.py:40-41), n floats, in place allowed.  The expm1
 * is evaluated as torch evaluates it on the CPU, where the reference decodes (a float-float sequence of fp32 adds, multiplies and
 * fmas), not with the device library's expm1f: bit-identical to the reference's decoded means, and the one function every decode
 * here shares (gs_decode_splats, gs_decode_dynamic_splats, compression.inverse_log_transform). */
int32_t gs_inverse_log_transform(uint64_t n, const float *y, float *out, gs_stream_t stream);
/* Decode of a spacetime splat file (STGPngCompression, gsplat/compression/stg_compression.py:124-143) STRAIGHT INTO
 * render_dynamic()'s RAW parameter dict by one kernel: every attribute of the STG map dequantized with the arithmetic of
 * gs_grid_dequantize (bit-identical), the means followed by the inverse log transform; no activation, no quaternion
 * normalisation.  Attribute order (11): means(3, 16-bit) scales(3) quats(4) opacities(1) trbf_center(1) trbf_scale(1) motion(9)
 * omega(4) colors(3) features_dir(3) features_time(3): 38 bytes read and 35 floats written per splat.
 *   planes14 (HOST array of 14 device pointers, [n, C] row-major uint8 each): means_l means_u scales quats opacities
 *     trbf_center trbf_scale motion motion_1 motion_2 omega colors features_dir features_time.  The motion is either ONE
 *     joined [n, 9] plane (motion_1 = motion_2 = NULL) or the three [n, 3] images of the file.  features_dir / features_time
 *     are optional: a NULL plane skips the attribute.
 *   mins35 / maxs35 (HOST): the per-channel bounds of meta.json in attribute order; bits11 (HOST): bit depth per attribute,
 *     means = 16, the others 1..8 (value in the top bits of the byte); outs11 (HOST array of 11 device pointers): [n, C] fp32.
 * n = 0 returns 0 without touching any pointer.  Queued on `stream`, no host wait. */
int32_t gs_decode_dynamic_splats(
    uint64_t n, const uint8_t *const *planes14, const float *mins35, const float *maxs35, const uint32_t *bits11,
    float *const *outs11, gs_stream_t stream);
/* K-means codebook decode of the higher SH bands (png_compression.py:487-520): out[r, :] =
 * centroids_quant[labels[r], :] / (2^bits - 1) * (maxs - mins) + mins (float64 arithmetic like the reference).
 * labels are file contents: one outside [0, n_centroids) (where the reference's centroids[labels] raises IndexError)
 * decodes to a NaN row and is counted in *n_bad (device uint32, zero-filled by the caller; may be NULL). */
int32_t gs_kmeans_decode(uint64_t n_rows, uint32_t width, const int32_t *labels, const uint8_t *centroids_quant,
                         uint32_t n_centroids, uint32_t bits, float mins, float maxs, float *out, uint32_t *n_bad,
                         gs_stream_t stream);
/* PNG scanline reconstruction, HOST code (PNG specification section 9: filter types 0..4): data = h rows of 1 + stride bytes
 * (filter type, filtered scanline), out = h rows of stride bytes, bpp = bytes per pixel.  The sequential part of reading the
 * image grids the reference writes through imageio (gsplat/compression/png_compression.py:196, 271, 344-349). */
int32_t gs_png_unfilter(const uint8_t *data, uint32_t h, uint32_t stride, uint32_t bpp, uint8_t *out);


/* ------------------------------------------------------------------------
 * Entropy coder of the on-disk format (ans.hip): a static, table-based, byte-wise rANS coder over MANY independent streams, one
 * GPU lane per stream -- what EntropyCodingCompression (gsplat/compression/entropy_coding_compression.py:328-446) takes from the
 * `constriction` package, behind a bitstream of this project's own whose definition is the numpy coder
 * gscodec_studio_amd/compression/ans_reference.py (the kernels' output is byte-identical to it).
 *   state 32 bits, lower bound 2^23, renormalised one byte at a time; probability resolution 2^P, 8 <= P <= 14;
 *   channel c of the N symbols (8 bits each) is cut into n_streams = ceil(N / S) streams of S symbols, stream k = symbols
 *   [k S, min(N, (k + 1) S)); stream index sid = c * n_streams + k; a stream is encoded last symbol first, so it decodes forward.
 * All of that -- state machine, stream geometry, the slot writer, the bounded reader -- is one stream layer (ans_stream_dev.h) that
 * the Gaussian route below runs too; this section's model is a static table per channel.
 * freq / cum: uint32 [C, 256] integer frequencies (sum 2^P per channel) and their exclusive prefix sums, derived on the host.
 *
 * gs_ans_histogram: symbols uint8 [N, C] -> counts uint32 [C, 256] (ADDED to: the caller zero-fills), LDS histogram per
 *   workgroup and one flush of atomics per workgroup; channel_major (uint8 [C, N], may be NULL) receives the transposed copy
 *   the encoder streams through.  C <= 16.
 * gs_ans_encode: each lane walks its stream backwards and writes its renormalisation bytes to the END of its slot of
 *   gs_ans_slot_bytes(S, P) = ceil(S P / 8) + 8 bytes (the worst case) in scratch (>= gs_ans_encode_bytes); lengths [C n_streams]
 *   = bytes written, states = final state; the bytes of stream sid are scratch[(sid + 1) slot - lengths[sid], (sid + 1) slot), in
 *   the order the decoder consumes them.  *status (device uint32, zero-filled by the caller) gets bit 0 set when a symbol with
 *   frequency 0 was met and bit 1 when a slot was too small (neither write leaves the slot).
 * gs_ans_pack_slots: after an exclusive scan of (4 + lengths) into offsets (int64 [n + 1], device): payload[offsets[sid]...] = the
 *   little-endian final state, then the stream's bytes, out of slots of slot_bytes each -- the one pack launch, for either model.
 *   A stream that would not fit payload_bytes is skipped.  gs_ans_pack: the same with slot_bytes = gs_ans_slot_bytes(S, P).
 * gs_ans_decode: payload + offsets (int64 [C n_streams + 1], device) -> symbols uint8 [N, C] (the layout gs_grid_dequantize
 *   reads).  Every read is bounded to the stream's byte range clamped to [0, payload_bytes]; beyond it the byte is 0: a damaged
 *   file decodes to wrong symbols, never to an out-of-range access.  P <= 14: the slot-to-symbol table (2^P bytes) lives in LDS. */
uint32_t gs_ans_slot_bytes(uint32_t S, uint32_t P);
uint64_t gs_ans_encode_bytes(uint64_t N, uint32_t C, uint32_t S, uint32_t P);
int32_t gs_ans_histogram(uint64_t N, uint32_t C, const uint8_t *symbols, uint32_t *counts, uint8_t *channel_major,
                         gs_stream_t stream);
int32_t gs_ans_encode(uint64_t N, uint32_t C, uint32_t S, uint32_t P, const uint8_t *channel_major, const uint32_t *freq,
                      const uint32_t *cum, uint8_t *scratch, uint64_t scratch_bytes, uint32_t *lengths, uint32_t *states,
                      uint32_t *status, gs_stream_t stream);
int32_t gs_ans_pack(uint64_t n_streams_total, uint32_t S, uint32_t P, const uint8_t *scratch, const uint32_t *lengths,
                    const uint32_t *states, const int64_t *offsets, uint8_t *payload, uint64_t payload_bytes, gs_stream_t stream);
int32_t gs_ans_decode(uint64_t N, uint32_t C, uint32_t S, uint32_t P, const uint8_t *payload, uint64_t payload_bytes,
                      const int64_t *offsets, const uint32_t *freq, const uint32_t *cum, uint8_t *symbols, gs_stream_t stream);
int32_t gs_ans_pack_slots(uint64_t n_streams_total, uint32_t slot_bytes, const uint8_t *scratch, const uint32_t *lengths,
                          const uint32_t *states, const int64_t *offsets, uint8_t *payload, uint64_t payload_bytes, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * Hash-grid Gaussian route of the entropy coder (gauss_ans.hip): the stream layer of the section above (ans_stream_dev.h) at
 * P = 16, under another model: EVERY SYMBOL HAS ITS OWN FREQUENCIES, given by mu_q (the mean on a grid of 8 steps per symbol, 0..2040) and k (a scale
 * level, 0..63: sigma_k = 2^((k - 22) / 5) symbol widths) through one table G uint16 [64, 4073]:
 *   cum(0) = 0, cum(256) = 2^16, cum(s) = G[k][clamp(8 s - 4 - mu_q, -2036, 2036) + 2036] + s for s = 1..255, f(s) = cum(s + 1) - cum(s)
 * (every f >= 1: any model codes any symbol).  The format's definition is gscodec_studio_amd/compression/gauss_ans_reference.py,
 * which also builds G and the 63 level thresholds; the kernels' output is byte-identical to it.
 *
 * gs_gauss_ans_params: one lane per splat; features float [N, 48] (gs_hashgrid_encode_fwd's output, read in place, 16-byte
 *   aligned) through Linear(48, 5C) [w1 [5C, 48], b1], ReLU (h > 0 ? h : 0), Linear(5C, 2C) [w2 [2C, 5C], b2] in float32 with the
 *   accumulator starting at the bias, inputs ascending, every product and sum rounded on its own; miu = out[c], sigma = out[C + c]
 *   (1e-9 where below); mu_norm = (miu - mins) / (maxs - mins) * 255, sigma_norm = sigma / (maxs - mins) * 255; mu_q = 0 where not
 *   mu_norm > 0, 2040 where mu_norm >= 255, else rint(8 mu_norm); k = the number of thresholds [63] <= sigma_norm.  Writes mu_q
 *   int16 [C, N] and k uint8 [C, N] (channel-major, what the coder reads); miu / sigma (float [N, C], may be NULL) receive the
 *   float values.  Inference only.  1 <= C <= 8.
 * gs_gauss_ans_encode: as gs_ans_encode, on channel_major symbols uint8 [C, N] (the transposed symbols); slots of
 *   gs_gauss_ans_slot_bytes(S) = 2 S + S / 512 + 8 bytes (the worst case at P = 16 plus 8) in scratch (>= gs_gauss_ans_encode_bytes);
 *   gs_ans_pack_slots copies them.  *status (device uint32, zero-filled by the caller): bit 0 = a mu_q or k out of range was met
 *   (clamped), bit 1 = a slot was too small (no write leaves the slot).  table: G on the device, 2-byte aligned.
 * gs_gauss_ans_decode: payload + offsets (int64 [C n_streams + 1], device) -> symbols uint8 [N, C].  Reads are bounded to the
 *   stream's byte range clamped to [0, payload_bytes], a byte beyond it is 0; mu_q, k and the table index are clamped; the symbol
 *   is found by an 8-step binary search and at most two bytes are read per symbol: a damaged file decodes to wrong symbols.
 * C <= 16 for the two coder entries. */
uint32_t gs_gauss_ans_slot_bytes(uint32_t S);
uint64_t gs_gauss_ans_encode_bytes(uint64_t N, uint32_t C, uint32_t S);
int32_t gs_gauss_ans_params(uint64_t N, uint32_t C, const float *features, const float *w1, const float *b1, const float *w2,
                            const float *b2, const float *mins, const float *maxs, const float *thresholds, int16_t *mu_q,
                            uint8_t *k, float *miu, float *sigma, gs_stream_t stream);
int32_t gs_gauss_ans_encode(uint64_t N, uint32_t C, uint32_t S, const uint8_t *channel_major, const int16_t *mu_q, const uint8_t *k,
                            const uint16_t *table, uint8_t *scratch, uint64_t scratch_bytes, uint32_t *lengths, uint32_t *states,
                            uint32_t *status, gs_stream_t stream);
int32_t gs_gauss_ans_decode(uint64_t N, uint32_t C, uint32_t S, const uint8_t *payload, uint64_t payload_bytes,
                            const int64_t *offsets, const int16_t *mu_q, const uint8_t *k, const uint16_t *table, uint8_t *symbols,
                            gs_stream_t stream);

/* ------------------------------------------------------------------------
 * Transform-coded attribute planes (plane_codec.hip): the payload of HevcCompression's <name>.bin -- a small intra codec for 8-bit
 * planes [H, W, ch] (ch = 1..4) under HEVC's quantisation parameter qp (0..51), in place of the reference's ffmpeg / libx265 call
 * (gsplat/compression/hevc_compression.py).  Not an HEVC stream: HEVC's 8-point integer transform and flat quantiser, no prediction,
 * no RDO, rANS (the stream layer above, ans_stream_dev.h) over 15 static tables.  The format's definition is
 * gscodec_studio_amd/compression/plane_codec_reference.py; integer arithmetic only, the kernels' results equal it element for
 * element.  n_blocks = ceil(H / 8) ceil(W / 8); levels int16 [ch, n_blocks, 64], 16-byte aligned, the 64 of a block in scan order.
 *
 * gs_plane_transform_fwd: plane uint8 [H, W, ch] -> levels: one lane per 8 x 8 block of one channel, coordinates clamped into the
 *   plane (edge replication), transform along x then y, quantiser.
 * gs_plane_transform_inv: levels (any values: clamped to +-32767) -> plane uint8 [H, W, ch] (the layout gs_grid_dequantize reads):
 *   dequantiser, transform along y then x, clip, only the pixels inside the plane are stored.
 * gs_plane_ans_encode: the flat symbols uint8 [N] (N = 64 ch n_blocks, ordered channel, block, scan position) as ONE channel of
 *   streams of S symbols, one lane per stream; the model of symbol i is row CTX[i % 64] (the anti-diagonal of its scan position) of
 *   cum uint16 [15, 257] (cumulative frequencies, cum[c][256] = 2^P, 8 <= P <= 14; kept in LDS).  Slots of
 *   gs_plane_ans_slot_bytes(S, P) = ceil(S P / 8) + 8 bytes in scratch (>= n_streams slots), lengths / states [n_streams];
 *   gs_ans_pack_slots copies them.  *status (device uint32, zero-filled by the caller): bit 0 = a symbol with frequency 0 was met,
 *   bit 1 = a slot was too small (no write leaves the slot).
 * gs_plane_ans_decode: payload + offsets (int64 [n_streams + 1], device) -> symbols uint8 [N].  Reads are bounded to the stream's
 *   byte range clamped to [0, payload_bytes], a byte beyond it is 0; the symbol is found by an 8-step binary search and at most two
 *   bytes are read per symbol: a damaged file decodes to wrong symbols. */
uint32_t gs_plane_ans_slot_bytes(uint32_t S, uint32_t P);
int32_t gs_plane_transform_fwd(uint32_t H, uint32_t W, uint32_t ch, uint32_t qp, const uint8_t *plane, int16_t *levels,
                               gs_stream_t stream);
int32_t gs_plane_transform_inv(uint32_t H, uint32_t W, uint32_t ch, uint32_t qp, const int16_t *levels, uint8_t *plane,
                               gs_stream_t stream);
int32_t gs_plane_ans_encode(uint64_t N, uint32_t S, uint32_t P, const uint8_t *symbols, const uint16_t *cum, uint8_t *scratch,
                            uint64_t scratch_bytes, uint32_t *lengths, uint32_t *states, uint32_t *status, gs_stream_t stream);
int32_t gs_plane_ans_decode(uint64_t N, uint32_t S, uint32_t P, const uint8_t *payload, uint64_t payload_bytes,
                            const int64_t *offsets, const uint16_t *cum, uint8_t *symbols, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * Transform-coded plane SEQUENCES (plane_codec.hip): the payload of SeqHevcCompression's <name>.bin -- T planes uint8 [T, H, W, ch]
 * with temporal prediction, in place of the reference's ffmpeg / libx265 call on a video of attribute grids
 * (gsplat/compression/seq_hevc_compression.py).  The format's definition is
 * gscodec_studio_amd/compression/plane_seq_codec_reference.py; the stages (transform, quantiser, dequantiser, inverse, scan) are the
 * plane codec's above, integer arithmetic only, the kernels' results equal the module element for element.  Frame t is an I frame
 * when t % gop == 0 (its levels are gs_plane_transform_fwd's), otherwise a P frame: the levels of the difference between the
 * edge-replicated source block and the padded reconstruction of frame t - 1 (all 64 pixels of every block, values 0..255), which
 * then becomes clip(reconstruction + inverse(levels), 0, 255).  No motion search and no spatial prediction: a block depends on the
 * co-located block alone, so ONE LANE OWNS ONE 8 x 8 BLOCK of one channel THROUGH ALL T FRAMES, with the reconstruction in
 * registers (64 bytes packed into 16 words); one launch runs the whole closed loop.  levels int16 [T, ch, n_blocks, 64], 16-byte
 * aligned, T ch n_blocks 64 < 2^31.
 *
 * gs_plane_seq_fwd: planes -> levels, and the decoder's frames into recon uint8 [T, H, W, ch] when recon is not NULL (cropped).
 * gs_plane_seq_inv: levels (any values: clamped to +-32767) -> planes uint8 [T, H, W, ch]: the second half of gs_plane_seq_fwd. */
int32_t gs_plane_seq_fwd(uint32_t T, uint32_t gop, uint32_t H, uint32_t W, uint32_t ch, uint32_t qp, const uint8_t *planes,
                         int16_t *levels, uint8_t *recon /* or NULL */, gs_stream_t stream);
int32_t gs_plane_seq_inv(uint32_t T, uint32_t gop, uint32_t H, uint32_t W, uint32_t ch, uint32_t qp, const int16_t *levels,
                         uint8_t *planes, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * Grid sort (grid_sort.hip): the order of the splats on the S x S image grid of the PNG codecs that makes every attribute image
 * smooth -- the role of the `plas` package in the reference (gsplat/compression/sort.py), as an algorithm of this project's own
 * whose definition is the numpy code gscodec_studio_amd/compression/grid_sort_reference.py.  Integer arithmetic only: the
 * kernels' results equal the reference's element for element.  N = S * S < 2^31, 1 <= C <= 64 channels of 12-bit features
 * q uint16 [N, C] (values <= 4095); order int32 [N]: order[p] = the splat at grid position p = y * S + x.  One round is
 * gs_gridsort_blur -> gs_gridsort_keys -> gs_sort_pairs_u64_i32 over bits [0, 32 + bits of the largest block id) ->
 * gs_gridsort_assign; every launch goes to `stream`, nothing waits on the host.
 *
 * gs_gridsort_blur: target[p] = the box blur of width 2 r + 1 (1 <= r < S, reflect borders) of the grid q[order[.]], rows
 *   first (into tmp), then columns, each pass an exact integer window sum s followed by (2 s + w) / (2 w).  tmp and target:
 *   uint16 [N, C].  One sliding window per (line, channel, segment of at most 128 outputs).
 * gs_gridsort_keys: keys[p] = block(p) << 32 | hash(seed, k, p), vals[p] = p.  Block side b >= 1, shifted by
 *   (hash(seed, k, N) % b, hash(seed, k, N + 1) % b): block(p) = ((y + oy) / b) (S / b + 2) + (x + ox) / b.  b = 0: no blocks,
 *   the key is the hash alone (the start order).
 * gs_gridsort_assign: one lane per run of four sorted positions.  Four positions of one block: the first of the 24
 *   permutations in lexicographic order whose sum of squared distances between the four items q[order_in[.]] and the four
 *   targets is least moves item i to position perm[i] of the run; any other run (and the trailing N % 4 positions) keeps its
 *   entries.  order_out (must not alias order_in) receives every position exactly once. */
int32_t gs_gridsort_blur(uint32_t S, uint32_t C, uint32_t r, const uint16_t *q, const int32_t *order, uint16_t *tmp,
                         uint16_t *target, gs_stream_t stream);
int32_t gs_gridsort_keys(uint32_t S, uint32_t b, uint32_t seed, uint32_t k, int64_t *keys, int32_t *vals, gs_stream_t stream);
int32_t gs_gridsort_assign(uint32_t S, uint32_t C, const uint16_t *q, const uint16_t *target, const int64_t *sorted_keys,
                           const int32_t *sorted_pos, const int32_t *order_in, int32_t *order_out, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * K-means codebook (kmeans.hip): the Lloyd steps behind the shN codec -- the role of `torchpq.clustering.KMeans` (manhattan
 * distance) in the reference (gsplat/compression/png_compression.py:420-484), as an algorithm of this project's own whose
 * definition is the numpy code gscodec_studio_amd/compression/kmeans_reference.py.  Integer arithmetic only: the kernels'
 * results equal the reference's element for element.  1 <= n < 2^31 points of 1 <= w <= 64 channels, 1 <= k <= 2^20 clusters;
 * q int32 [w, n] (channel-major), values in [0, 2^24 - 1]; cent int32 [k, wp] with wp = gs_kmeans_padded_width(w) (the next of
 * 4, 8, 16, 32, 48, 64; 0 for a w outside 1..64) and the channels w <= c < wp ZERO: the caller zero-fills them once, nothing
 * here writes them.  Every launch goes to `stream`, nothing waits on the host.
 *
 * gs_kmeans_assign: labels[i] = the lowest j with the least d(i, j) = sum over c of |q[c, i] - cent[j, c]| (< 2^30), and
 *   n_changed[0] = the number of i whose label differs from the one labels[i] held on entry (labels is read, then written; the
 *   counter is zeroed here).  k_slices (1 <= k_slices <= min(k, 65535)) cuts the centroids into that many slices walked by
 *   different workgroups that meet in a 64-bit atomic minimum over d << 32 | j in keys uint64 [n] (may be NULL with one slice);
 *   the labels do not depend on it.  gs_kmeans_default_slices: one slice when n alone fills the chip, otherwise as many as
 *   bring the grid to about four workgroups per CU, of 64 centroids at least (0 for a shape outside the bounds above).
 * gs_kmeans_update: sums[j, c] = the sum of q[c, i] over labels[i] == j (uint64 [k, w], scratch), counts[j] = their number
 *   (uint32 [k], left for the caller to read), cent[j, c] = (2 sums + counts) / (2 counts) for c < w where counts[j] > 0; the
 *   centroid of an empty cluster is not written.  A label outside [0, k) adds nowhere. */
uint32_t gs_kmeans_padded_width(uint32_t w);
uint32_t gs_kmeans_default_slices(uint32_t n, uint32_t w, uint32_t k);
int32_t gs_kmeans_assign(uint32_t n, uint32_t w, uint32_t k, const int32_t *q, const int32_t *cent, uint32_t k_slices,
                         uint64_t *keys, int32_t *labels, uint32_t *n_changed, gs_stream_t stream);
int32_t gs_kmeans_update(uint32_t n, uint32_t w, uint32_t k, const int32_t *q, const int32_t *labels, uint64_t *sums,
                         uint32_t *counts, int32_t *cent, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * Nearest neighbours (knn.hip): the exact K nearest points of 3-D float32 points -- the role of `knn` in the reference's trainers
 * (examples/utils.py:142-146: sklearn's NearestNeighbors on the host), as an algorithm of this project's own whose definition is
 * the numpy code gscodec_studio_amd/knn_reference.py: a uniform grid of rx x ry x rz cells of side h from the corner lo (`box`: four
 * float64 in HOST memory, lo x, y, z and h, read during the call; 1 <= r <= 1024 per axis, h > 0), the cell of a point
 * clamp(floor((double(p) - lo) / h), 0, r - 1) per axis, its id (cz ry + cy) rx + cx; border cells reach to infinity.
 * 1 <= n, m < 2^31.  The host chooses lo, h and r (knn_reference.cell_size) and sorts (cell id, index) between the first two
 * calls (gs_sort_pairs_u64_i32 over the bits of the largest id).  Every launch goes to `stream`, nothing waits on the host, no
 * atomics.
 *
 * gs_knn_cells: cell_ids[i] = the id of xyz[i] (float [n, 3]), ids[i] = i: the pairs to sort.
 * gs_knn_finish_grid: sorted_xyzi float [n, 4] (16-byte aligned) = (xyz[order[p]], the bits of order[p]) for every position p;
 *   and, with ncells > 0, cell_starts int32 [ncells + 1]: cell_starts[c] = the number of sorted_ids below c (ncells = 0: the
 *   sorted copy of a query list, sorted_ids and cell_starts may be NULL).
 * gs_knn_search: for the m queries of queries_xyzi float [m, 4] (xyz and, as bits in w, the row < m each result goes to; in
 *   cell-sorted order for speed, any order for the result; the same array as sorted_xyzi for the neighbours of the points
 *   themselves), the K (1 <= K <= min(16, n)) points of sorted_xyzi with the least (d^2, index), d^2 = (dx dx + dy dy) + dz dz in
 *   float32 without contraction: dist float [m, K] = sqrtf(d^2) ascending, idx int64 [m, K] (both or neither), and / or
 *   log_scales float [m, 3] = log(sqrt(mean of d^2 over columns 1 .. K - 1) * init_scale) in every column (K >= 2; the mean
 *   and what follows in float64; -inf where the mean is zero).  The kernel is instantiated for K padded to 4, 8 and 16. */
int32_t gs_knn_cells(uint32_t n, const float *xyz, const double *box, uint32_t rx, uint32_t ry, uint32_t rz, int64_t *cell_ids,
                     int32_t *ids, gs_stream_t stream);
int32_t gs_knn_finish_grid(uint32_t n, uint32_t ncells, const float *xyz, const int64_t *sorted_ids, const int32_t *order,
                           float *sorted_xyzi, int32_t *cell_starts, gs_stream_t stream);
int32_t gs_knn_search(uint32_t n, uint32_t m, uint32_t K, const float *sorted_xyzi, const int32_t *cell_starts,
                      const float *queries_xyzi, const double *box, uint32_t rx, uint32_t ry, uint32_t rz, float *dist,
                      int64_t *idx, float *log_scales, float init_scale, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * PLY splat files (ply.hip): the vertex rows of a `binary_little_endian 1.0` .ply in the INRIA 3DGS layout -- what the reference
 * reads and writes on the host through the plyfile package (examples/simple_trainer.py:414-510 save_ply / load_ply) -- to and
 * from the six splat tensors, by one kernel each way.  `rows`: n rows of `stride` bytes (1 <= stride <= gs_ply_max_stride() =
 * 1024), DEVICE memory, 16-byte aligned.  The tensors are six groups in the order means, sh0, shN, opacities, scales, quats:
 * widths6 (HOST, six counts of floats per row; 0: no such tensor, its pointer is not looked at) and outs6 / ins6 (HOST array of
 * six DEVICE pointers, float [n, width] each).  cols (HOST, sum of the widths <= gs_ply_max_columns() = 128 entries): for every
 * float of a row of group 0, then of group 1, ..., the byte offset inside the file's row it comes from (bits 0..15), bit 16 set
 * for a `double` column (read as float64, rounded to float32 to nearest even), every other bit zero.  The caller builds the
 * table from the file's header, so property order, skipped columns and the channel-major f_dc_* / f_rest_* to [K, 3]
 * transposition are all in the table.  A workgroup stages gs_ply_block_rows(stride) rows (256, 128 or 64: the most that fit
 * 64 KB) in LDS; both sides of the transposition are contiguous in global memory.
 *
 * gs_ply_unpack: rows -> tensors.  activate = 1: group 4 (scales) = exp(.), group 3 (opacities) = sigmoid(.);
 *   normalize_quats = 1: group 5 (quats) = q / max(||q||, 1e-12) -- the arithmetic of gs_decode_splats.  With both 0 every
 *   float column is a move of bits (NaN payloads, -0 and denormals survive).  Offsets and stride all multiples of 4: word
 *   reads from LDS; anything else, or force_bytes = 1: byte-wise assembly.
 * gs_ply_pack: tensors -> rows; float columns only, stride and offsets multiples of 4, no two entries the same offset; bytes of
 *   a row that no entry covers are written as zero.
 * Both return a status without launching for a null pointer, n = 0 or n >= 2^31, a stride of 0 or above the limit, rows that
 * are not 16-byte aligned, too many columns, an unknown flag bit or an offset whose value does not end inside the stride.
 * Queued on `stream`, no host wait. */
uint32_t gs_ply_max_stride(void);
uint32_t gs_ply_max_columns(void);
uint32_t gs_ply_block_rows(uint32_t stride); /* 0 for a stride outside 1 .. gs_ply_max_stride() */
int32_t gs_ply_unpack(uint32_t n, uint32_t stride, const uint8_t *rows, const uint32_t *cols, const uint32_t *widths6,
                      float *const *outs6, int32_t activate, int32_t normalize_quats, int32_t force_bytes, gs_stream_t stream);
int32_t gs_ply_pack(uint32_t n, uint32_t stride, const uint32_t *cols, const uint32_t *widths6, const float *const *ins6,
                    uint8_t *rows, gs_stream_t stream);


/* ------------------------------------------------------------------------
 * accumulate (reference gsplat/cuda/_torch_impl.py:432-519, exported as gsplat.accumulate): alpha compositing over an explicit list
 * of M (gaussian, pixel, camera) intersections -- the output of the rasterize_indices pair above: grouped by ray (camera, pixel),
 * front to back inside a ray.  alpha = min(opacity exp(-sigma), 0.999); weight = alpha x the product of (1 - alpha) over the
 * entries in front of it in its run (nerfacc.render_weight_from_alpha); renders[camera, pixel] += sum weight colour,
 * alphas[camera, pixel] += sum weight (nerfacc.accumulate_along_rays).  A run = consecutive entries with the same (camera, pixel).
 * renders [C,H,W,channels] / alphas [C,H,W] are ADDED to (the caller zero-fills them); alpha_buf / weights [M] are written and
 * handed back to gs_accumulate_bwd, which ADDS into v_means2d [C,N,2], v_conics [C,N,3], v_opacities [C,N], v_colors
 * [C,N,channels] (float atomics; each may be NULL) and uses v_alpha_pair [M] as scratch.  v_renders / v_alphas may be NULL. */
int32_t gs_accumulate_fwd(uint64_t M, uint32_t C, uint32_t N, uint32_t channels, const float *means2d, const float *conics,
                          const float *opacities, const float *colors, const int64_t *gaussian_ids, const int64_t *pixel_ids,
                          const int64_t *camera_ids, int32_t image_width, int32_t image_height, float *alpha_buf, float *weights,
                          float *renders, float *alphas, gs_stream_t stream);
int32_t gs_accumulate_bwd(uint64_t M, uint32_t C, uint32_t N, uint32_t channels, const float *means2d, const float *conics,
                          const float *opacities, const float *colors, const int64_t *gaussian_ids, const int64_t *pixel_ids,
                          const int64_t *camera_ids, int32_t image_width, int32_t image_height, const float *alpha_buf,
                          const float *weights, const float *v_renders, const float *v_alphas, float *v_alpha_pair,
                          float *v_means2d, float *v_conics, float *v_opacities, float *v_colors, gs_stream_t stream);

/* Accumulated depth -> expected depth, the image-level tail of rasterization()'s "ED" / "RGB+ED" render modes
 * (gsplat/rendering.py:471-477): out = cat(renders[..., :-1], renders[..., -1:] / alphas.clamp(min=1e-10)) over n_pix pixels of
 * `channels` floats, one pass each way instead of slice / clamp / div / cat and their autograd twins.  bwd: v_renders[..., :-1] =
 * v_out[..., :-1], v_renders[..., -1] = v_out[..., -1] / clamp(alpha), v_alphas = -v_out[..., -1] ((renders[..., -1] / clamp) / clamp)
 * where alpha >= 1e-10, else 0 (torch's div and clamp derivatives); either output may be NULL. */
int32_t gs_expected_depth_fwd(uint64_t n_pix, uint32_t channels, const float *renders, const float *alphas, float *out, gs_stream_t stream);
int32_t gs_expected_depth_bwd(uint64_t n_pix, uint32_t channels, const float *renders, const float *alphas, const float *v_out,
                              float *v_renders, float *v_alphas, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * Temporal slicing of dynamic (spacetime) gaussians at one timestamp: the elementwise
 * chain in front of rasterization() in examples/simple_trainer_dyngs.py:506-521 -- trbf opacity decay
 * exp(-((t - center) / (sqrt2 scale))^2), cubic motion of the means (motion [N,9] = linear | quadratic |
 * cubic coefficients), quats + (t - center) omega re-normalised (F.normalize, eps 1e-12).  t - center is
 * detached where it drives motion and rotation (as `tforpoly` is), so trbf_center / trbf_scale receive
 * gradient through the opacity only.  trbf (optional output) is what the caller thresholds (> 0.05) for
 * the temporal visibility mask.  bwd: every output pointer may be NULL (not needed); all are overwritten. */
int32_t gs_temporal_slice_fwd(
    uint32_t n, const float *means, const float *motion, const float *quats, const float *omega,
    const float *opacities, const float *trbf_center, const float *trbf_scale, float timestamp,
    float *means_t, float *quats_t, float *opacity_t, float *trbf /* or NULL */, gs_stream_t stream);
int32_t gs_temporal_slice_bwd(
    uint32_t n, const float *means, const float *motion, const float *quats, const float *omega,
    const float *opacities, const float *trbf_center, const float *trbf_scale, float timestamp,
    const float *v_means_t, const float *v_quats_t, const float *v_opacity_t, const float *v_trbf /* each or NULL */,
    float *v_means, float *v_motion, float *v_quats, float *v_omega, float *v_opacities,
    float *v_trbf_center, float *v_trbf_scale, gs_stream_t stream);

/* The spacetime trainer's nine colour channels in one pass each way (round 6; examples/simple_trainer_STG.py:506-551):
 *     out[n] = (colors[n] | features_dir[n] | (timestamp - trbf_center[n]) * features_time[n]),   [N,9] from three [N,3]
 * replacing torch.cat + the tforpoly multiply (and autograd's split + copies on the way back).  quant_mask bit p (0 colors, 1
 * features_dir, 2 features_time): that part first goes through the round-to-grid STE hook of the compression simulation
 * (gsplat/compression_simulation/ops.py:57-75 with q_type "round": the PARAMETER is clamped in place to [lo, hi], the value used is
 * round((x - lo) / range / step_norm) * step_norm * range + lo with range = hi - lo, step_norm = 1 / (2^bits - 1), as
 * gs_quantize_round_fwd computes it); tables of 3 floats each, NULL with quant_mask 0.  bwd: the hook's gradient is the identity;
 * v_features_time = (timestamp - trbf_center) * v_out[:, 6:9]; trbf_center receives none (tforpoly is detached).  Output pointers of
 * bwd may be NULL (not needed). */
int32_t gs_stg_features_fwd(
    uint32_t n, float *colors, float *features_dir, float *features_time, const float *trbf_center, float timestamp,
    uint32_t quant_mask, const float *quant_lo, const float *quant_hi, const float *quant_range, const float *quant_step_norm,
    float *out, gs_stream_t stream);
int32_t gs_stg_features_bwd(
    uint32_t n, const float *v_out, const float *trbf_center, float timestamp, float *v_colors, float *v_features_dir,
    float *v_features_time, gs_stream_t stream);

/* The same slice evaluated INSIDE the row-form projection (round 6; SURVEY 8f rank 2: "folded into the projection kernel's load
 * phase"): gs_projection_rows_dyn_fwd == gs_temporal_slice_fwd followed by gs_projection_rows_fwd (colours [N,3] or none, no SH),
 * bit for bit -- the per-splat arithmetic is one shared definition (csrc/dynamic_dev.h, projection_dev.h) -- without the round trip of
 * means_t / quats_t / opacity_t through HBM; gs_projection_rows_dyn_bwd == gs_projection_rows_bwd followed by
 * gs_temporal_slice_bwd, writing the gradients of means, quats, scales, motion, omega, trbf_center, trbf_scale, opacities (and colors)
 * for the gaussians some camera saw (outputs_prefilled != 0: the other rows hold zeros already and are not stored; 0: every row is
 * written).  Opt-in on top, so that the trainer's RAW parameters can be handed over as they are (simple_trainer_dyngs.py:493-505):
 *   raw_params   GS_DYN_RAW_* bits: scales are log-scales (exp), opacities logits (sigmoid), trbf_scale a log-scale (exp) -- the
 *                activation runs in the kernel, its derivative in the backward;
 *   quant_mask   bit 0 scales, 1 quats, 2 opacities, 3 colors: the attribute goes through the STE round quantizer first
 *                (gsplat/compression_simulation/ops.py:57-75, the arithmetic of gs_quantize_round_fwd bit for bit): clamp to
 *                [quant_lo[k], quant_hi[k]] -- stored back into the PARAMETER when it changes a value, as the reference's in-place
 *                clamp does, which is why quats / scales / opacities / colors are not const in the forward --, round to the grid
 *                (quant_range[k] = hi - lo, quant_step_norm[k] = 1 / (2^bits - 1), both computed as the reference does: python
 *                double, then float), identity gradient.  The four tables are HOST arrays of 4 floats (NULL with quant_mask 0).
 * colors NULL: the colour columns of the rows are left to the caller (more than three render channels). */
#define GS_DYN_RAW_SCALES 1u
#define GS_DYN_RAW_OPACITIES 2u
#define GS_DYN_RAW_TRBF_SCALE 4u
int32_t gs_projection_rows_dyn_fwd(
    uint32_t C, uint32_t N, const float *means, float *quats, float *scales, const float *motion, const float *omega,
    const float *trbf_center, const float *trbf_scale, float timestamp,
    float min_trbf /* gaussians whose temporal basis is <= this are culled at this timestamp (the trainer's temp_vis_mask, 0.05); < 0: none */,
    uint8_t *trbf_alive /* [N] or NULL: 1 where trbf > min_trbf (the trainer's t_vis_mask) */,
    uint32_t raw_params, uint32_t quant_mask, const float *quant_lo,
    const float *quant_hi, const float *quant_range, const float *quant_step_norm, const float *viewmats, const float *Ks,
    int32_t image_width, int32_t image_height, float eps2d, float near_plane, float far_plane, float radius_clip, int32_t camera_model,
    float *opacities /* [N] or NULL */, float *colors /* [N,3] or NULL */, int32_t antialiased,
    uint32_t tile_size, uint32_t tile_width, uint32_t tile_height, int32_t *tiles_per_gauss /* or NULL */, int32_t *block_sums /* or NULL */,
    int32_t *radii, float *depths, float *rows, gs_stream_t stream);
int32_t gs_projection_rows_dyn_bwd(
    uint32_t C, uint32_t N, const float *means, const float *quats, const float *scales, const float *motion, const float *omega,
    const float *trbf_center, const float *trbf_scale, float timestamp, uint32_t raw_params, uint32_t quant_mask, const float *quant_lo,
    const float *quant_hi, const float *quant_range, const float *quant_step_norm, const float *viewmats, const float *Ks,
    int32_t image_width, int32_t image_height, float eps2d, int32_t camera_model, const int32_t *radii, const float *rows,
    const float *grad_rows, const float *v_depths /* or NULL */, const float *opacities, int32_t antialiased,
    float *v_means, float *v_quats, float *v_scales, float *v_motion, float *v_omega, float *v_trbf_center, float *v_trbf_scale,
    float *v_opacities, float *v_colors /* each or NULL */, int32_t outputs_prefilled, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * Row packing around the multi-GPU exchange of projected splats.  The gaussian-sharded mode of the reference
 * (gsplat/rendering.py:397-478, gsplat/distributed.py:170-257) concatenates radii | means2d | depths | conics |
 * opacities | colours with torch.cat before every all-to-all and splits them afterwards; these two replace the
 * cat / split: gs_rows_pack gathers the column blocks of up to 8 row-major arrays of 4-byte elements (part k:
 * device pointer parts[k] or NULL = zeros, widths[k] columns, row stride row_strides[k] elements, so column views
 * of wider buffers are read in place) into wire rows of sum(widths) elements; gs_rows_unpack scatters wire rows
 * back (NULL part = skipped).  parts / widths / row_strides are HOST arrays of n_parts entries. */
int32_t gs_rows_pack(
    uint64_t n_rows, int32_t n_parts, const void *const *parts, const int32_t *widths, const int64_t *row_strides,
    void *wire, gs_stream_t stream);
int32_t gs_rows_unpack(
    uint64_t n_rows, int32_t n_parts, void *const *parts, const int32_t *widths, const int64_t *row_strides,
    const void *wire, gs_stream_t stream);
/* Sparse form (only the rows of visible splats travel): wire row r pairs with row row_index[r * index_stride] of every
 * part whose indexed[k] flag (HOST array) is non-zero, and with row r of the others -- a gather on the way in, a scatter
 * on the way out.  row_index may alias a column of the wire itself (index_stride = wire width). */
int32_t gs_rows_pack_indexed(
    uint64_t n_rows, int32_t n_parts, const void *const *parts, const int32_t *widths, const int64_t *row_strides,
    const int32_t *indexed, const int32_t *row_index, int64_t index_stride, void *wire, gs_stream_t stream);
int32_t gs_rows_unpack_indexed(
    uint64_t n_rows, int32_t n_parts, void *const *parts, const int32_t *widths, const int64_t *row_strides,
    const int32_t *indexed, const int32_t *row_index, int64_t index_stride, const void *wire, gs_stream_t stream);
/* Compaction for the sparse form of that exchange: the rows with radii > 0 of radii [C_total, N] are listed per
 * destination rank d = c / C_local in a chunk of `cap` slots + 1 header row (slot order arbitrary):
 * src_index [world * (cap + 1)] = c * N + n or -1; hdr [world * (cap + 1), 2] = (row in the receiver's [C_local * N_total]
 * arrays, 0) or -1, header row = (-1, min(count, cap) | overflow << 30) where overflow = SOME chunk of this call was too small; counters [world] = rows wanted per destination;
 * stats [2] = (largest count, any overflow).  Both index arrays feed gs_rows_pack_indexed (a negative index packs
 * zeros / is skipped by gs_rows_unpack_indexed).  No read-back: `cap` comes from the caller's previous steps, and an
 * overflow is visible to every receiver in the header rows. */
int32_t gs_exchange_compact(
    uint32_t C_total, uint32_t N, uint32_t C_local, uint32_t world, uint32_t cap, uint32_t N_total, uint32_t N_off,
    const int32_t *radii, int32_t *src_index, int32_t *hdr, uint32_t *counters, uint32_t *stats, gs_stream_t stream);
/* The same exchange for SPLAT ROWS (gs_projection_rows_fwd): the 64-byte row IS the wire row, so nothing is packed or
 * split -- a row carries its radius (column 10) and depth (column 9), and columns 12 / 13 (padding) carry the two ints of
 * gs_exchange_compact's `hdr` (destination row | chunk header).
 * gs_rows16_gather: out_rows[r] = src_rows[index[r * index_stride]] (a negative index gives zeros); tag [n_rows,2] or NULL
 *   is stored into columns 12 / 13.  Forward: index = src_index, tag = hdr; backward: index = column 12 of the received
 *   rows (index_stride 16), src_rows = the gradient rows of gs_rasterize_bwd, tag = NULL.
 * gs_rows16_scatter: dst_rows[index[r * index_stride]] = wire_rows[r] where the index is >= 0; radii / depths (optional)
 *   receive columns 10 / 9 at the same element.  Forward: index = column 12 of the received rows; backward: src_index. */
int32_t gs_rows16_gather(
    uint64_t n_rows, const int32_t *index, int64_t index_stride, const float *src_rows, const int32_t *tag, float *out_rows,
    gs_stream_t stream);
int32_t gs_rows16_scatter(
    uint64_t n_rows, const int32_t *index, int64_t index_stride, const float *wire_rows, float *dst_rows, int32_t *radii,
    float *depths, gs_stream_t stream);
/* The two sides of that exchange as ONE call each (what distributed._ExchangeRows issues: the gaussian-sharded step is bound
 * by the host's launch work, every native call less counts):
 * gs_exchange_rows_send = gs_exchange_compact + gs_rows16_gather(src_index, hdr) into send_rows [world * (cap + 1), 16];
 *   src_index is kept for the backward, hdr / counters are scratch of the call.
 *   zero_radii (optional, [n_zero] int32): zero-filled by the call's first launch -- the RECEIVER-side radii of the same
 *   process, allocated before the all-to-all; gs_exchange_rows_recv(radii_zeroed = 1) then skips its own fill.
 * gs_exchange_rows_recv = zero-fill of radii [n_dst] + gs_rows16_scatter(index = column 12 of recv_rows) + gs_exchange_flags. */
int32_t gs_exchange_rows_send(
    uint32_t C_total, uint32_t N, uint32_t C_local, uint32_t world, uint32_t cap, uint32_t N_total, uint32_t N_off,
    const int32_t *radii, const float *rows, int32_t *src_index, int32_t *hdr, uint32_t *counters, uint32_t *stats,
    float *send_rows, int32_t *zero_radii, uint64_t n_zero, gs_stream_t stream);
int32_t gs_exchange_rows_recv(
    uint64_t n_recv, const float *recv_rows, uint64_t n_dst, float *dst_rows, int32_t *radii, float *depths,
    uint32_t world, const int64_t *hdr_rows, const uint32_t *stats, int32_t *out3, int32_t radii_zeroed, gs_stream_t stream);
/* After the all-to-all of those chunks: out3 = (some sender overflowed (bit 30 of the count in the header row hdr_rows[d] of
 * every received chunk; recv rows are row_width ints wide), stats[0], stats[1]).  out3 may be pinned HOST memory: the flags
 * then reach the host with the renderer's own tile-count read-back, without a copy command or a sync of their own. */
int32_t gs_exchange_flags(
    uint32_t world, const int32_t *recv, uint32_t row_width, const int64_t *hdr_rows, const uint32_t *stats, int32_t *out3,
    gs_stream_t stream);
/* ------------------------------------------------------------------------
 * Row gather and its adjoint for the packed (COO) pipeline: the torch indexing `opacities[gaussian_ids]`,
 * `colors[gaussian_ids]`, `means[gaussian_ids]` of gsplat/rendering.py:325, 365-380 and its backward (torch sorts the
 * ids and runs ~45 small kernels there).  src [*, width] fp32, ids int64 [n_rows]; gs_scatter_add_rows_f32 ADDS
 * v_out [n_rows, width] into v_src [*, width] (zero-fill first) with float atomics. */
int32_t gs_gather_rows_f32(
    uint64_t n_rows, uint32_t width, const float *src, const int64_t *ids, float *out, gs_stream_t stream);
int32_t gs_scatter_add_rows_f32(
    uint64_t n_rows, uint32_t width, const float *v_out, const int64_t *ids, float *v_src, gs_stream_t stream);
/* Plan of the sparse gradient reduction of the camera-sharded mode (distributed.py; no reference counterpart: the reference's
 * multi-GPU mode shards the gaussians).  gs_dp_visibility: vis[n] = any camera c with radii[c, n] > 0 (zeros behind N, up to
 * n_pad).  gs_dp_plan, from the all-gathered masks uint8 [world, n_pad = world * block] (splat n belongs to owner n / block):
 *   counts   int32 [world * world + world], ZERO-FILLED by the caller: rows[r][o] = splats of owner o that rank r saw, then
 *            urows[o] = splats of owner o that any rank saw;
 *   send_idx int32 [n_pad]: this rank's visible splats, ascending; urank int32 [n_pad]: position of every union splat in
 *            the ascending list of all union splats; uidx int32 [n_pad]: that list (entries behind the counts: undefined);
 *   tile_counts: scratch, 8 bytes x gs_dp_plan_tiles(n_pad).  world <= 16.
 * gs_dp_reduce_rows: the owner side of the reduction.  wire [n_recv, 1 + width] = the rows received from all senders (chunk
 * of sender k = rows [chunk_starts[k], chunk_starts[k + 1]), HOST array of world + 1 entries), column 0 the global splat index
 * as an int32 bit pattern (negative: no row).  Writes acc [umax, 1 + width]: row u = (uidx[u] for u < n_valid else -1 | scale *
 * sum of the received rows whose index maps to u, u = map[index] - map_offset) -- every row written once, no atomics, no
 * zero-fill.  inv: scratch, int32 [world * umax]. */
uint32_t gs_dp_plan_tiles(uint32_t n_pad);
int32_t gs_dp_visibility(uint32_t C, uint32_t N, uint32_t n_pad, const int32_t *radii, uint8_t *vis, gs_stream_t stream);
int32_t gs_dp_plan(uint32_t world, uint32_t rank, uint32_t n_pad, uint32_t block, const uint8_t *masks, void *tile_counts,
                   int32_t *counts, int32_t *send_idx, int32_t *urank, int32_t *uidx, gs_stream_t stream);
int32_t gs_dp_reduce_rows(uint64_t n_recv, uint32_t width, uint32_t world, const float *wire, const int64_t *chunk_starts,
                          const int32_t *map, int32_t map_offset, uint64_t umax, uint32_t n_valid, const int32_t *uidx, float scale,
                          int32_t *inv, float *acc, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * O1  Adam / SelectiveAdam over several tensors in ONE launch (the optimizer step after the render backward: one
 * torch.optim.Adam per splat attribute in the trainers, gsplat/optimizers/selective_adam.py with --visible_adam).  descs: HOST
 * array; more than GS_ADAM_MULTI_MAX descriptors are split over several launches on the same stream.  Every float array is
 * fp32, contiguous, 4-byte aligned, n floats; param, exp_avg and exp_avg_sq are updated in place.  Descriptors with n == 0 are
 * skipped.  No atomics: the results are bit-identical from run to run and do not depend on the grid.
 *   GS_ADAM_DENSE:     torch.optim.adam._single_tensor_adam (non-capturable, no weight decay / amsgrad / maximize), in its order
 *                      of operations: m = lerp(m, g, one_minus_beta1) (ATen's two-branch lerp); v = v * beta2;
 *                      v = v + (one_minus_beta2 * g) * g; p = p + (-step_size) * (m / (sqrt(v) / bias_correction2_sqrt + eps)).
 *                      The caller computes one_minus_beta1 = 1 - beta1, one_minus_beta2 = 1 - beta2, step_size = lr / (1 - beta1^step)
 *                      and bias_correction2_sqrt = (1 - beta2^step)^0.5 in double and rounds them to float, as torch does; it
 *                      also advances its step counter.  lr, rows, row_width and visibility are not read.
 *   GS_ADAM_SELECTIVE: gsplat/cuda/csrc/adam.cu:31-40 as written (no bias correction): m = beta1 * m + (1 - beta1) * g;
 *                      v = beta2 * v + ((1 - beta2) * g) * g; p += (-lr * m) / (sqrt(v) + eps), only for the elements e with
 *                      visibility[e / row_width] != 0 (uint8 / bool [rows]); the elements of the other rows are neither read nor
 *                      written.  n == rows * row_width < 2^32, row_width < 2^31.  one_minus_*, step_size and
 *                      bias_correction2_sqrt are not read. */
#define GS_ADAM_DENSE 0
#define GS_ADAM_SELECTIVE 1
#define GS_ADAM_MULTI_MAX 16
typedef struct gs_adam_desc {
    uint64_t n;                  /* floats in each of the four arrays (0: skipped) */
    float *param;                /* updated in place */
    const float *grad;
    float *exp_avg, *exp_avg_sq; /* updated in place */
    const uint8_t *visibility;   /* selective: [rows]; dense: not read */
    uint32_t rows, row_width;    /* selective: n = rows * row_width */
    float lr, beta1, beta2, eps;
    float one_minus_beta1, one_minus_beta2, step_size, bias_correction2_sqrt; /* dense */
    int32_t mode;                /* GS_ADAM_DENSE / GS_ADAM_SELECTIVE */
} gs_adam_desc;
uint32_t gs_adam_multi_max(void);
/* layout guard (see gs_step_layout): sizeof, then offsetof n, param, grad, exp_avg, exp_avg_sq, visibility, rows, row_width, lr,
 * step_size, mode */
uint32_t gs_adam_desc_layout(uint64_t *out, uint32_t n);
int32_t gs_adam_multi(uint32_t n_tensors, const gs_adam_desc *descs, gs_stream_t stream);

/* O2  SparseAdam over several tensors that share ONE index list, in one launch (torch.optim.SparseAdam per splat attribute in
 * the trainers' --sparse_grad mode: COO gradients over the packed render's gaussian_ids).  descs: HOST array; more than
 * GS_ADAM_MULTI_MAX descriptors are split over several launches on the same stream.  param, exp_avg, exp_avg_sq: fp32
 * [rows, row_width], updated in place; values: fp32 [nnz, row_width], the gradient's value rows; all contiguous, 4-byte aligned.
 * sorted_ids: int64 [nnz], ascending, every id in [0, rows) (an id outside is skipped, never used as an address).  perm: int32
 * [nnz], perm[k] = the row of `values` that sorted_ids[k] came from, or NULL = identity (a coalesced or already sorted gradient).
 * The rows whose id does not occur are neither read nor written.  Per element of the other rows,
 * torch.optim._functional.sparse_adam in its order of operations, one float32 rounding each:
 *   g = the sum of the duplicates' values;  d1 = (g - m) * one_minus_beta1;  d2 = (g * g - v) * one_minus_beta2;
 *   m = m + d1;  v = v + d2;  p = p + neg_step_size * ((d1 + m_old) / (sqrt(d2 + v_old) + eps))
 * The caller computes one_minus_beta1 = 1 - beta1, one_minus_beta2 = 1 - beta2 and neg_step_size =
 * -(lr * sqrt(1 - beta2^step) / (1 - beta1^step)) in double and rounds them to float, as torch does; it also advances its step
 * counter.  Duplicates: a run of equal ids is summed in the order of its positions in sorted_ids, starting from its first value;
 * with perm from a stable sort on (id, position) -- gs_sort_pairs_u64_i32 over (ids, 0 .. nnz - 1) -- that is ascending position
 * in `values`.  (torch's coalesce() sums three or more duplicates in another order; up to two, or exactly representable sums,
 * agree bit for bit.)  A run of length r costs r serial loads per column: meant for r <= the number of cameras.
 * nnz < 2^31, 1 <= row_width < 2^31, nnz * row_width < 2^32, rows * row_width < 2^32; all checked, with the null pointers and
 * the alignment, before anything is launched.  nnz == 0: nothing is launched.  No atomics: every (row, column) is written by one
 * lane, the results are bit-identical from run to run and do not depend on the grid. */
typedef struct gs_sparse_adam_desc {
    float *param;                /* [rows, row_width], updated in place */
    float *exp_avg, *exp_avg_sq; /* [rows, row_width], updated in place */
    const float *values;         /* [nnz, row_width] */
    uint32_t row_width;
    float one_minus_beta1, one_minus_beta2, neg_step_size, eps;
} gs_sparse_adam_desc;
/* layout guard (see gs_step_layout): sizeof, then offsetof param, exp_avg, exp_avg_sq, values, row_width, one_minus_beta1,
 * one_minus_beta2, neg_step_size, eps */
uint32_t gs_sparse_adam_desc_layout(uint64_t *out, uint32_t n);
int32_t gs_sparse_adam_multi(uint32_t n_tensors, const gs_sparse_adam_desc *descs, uint64_t nnz, const int64_t *sorted_ids,
                             const int32_t *perm, uint64_t rows, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * L1  The trainers' photometric loss: the 3DGS SSIM of the fused_ssim package (11-tap separable Gaussian window, sigma 1.5,
 * zero padding, C1 = 0.01^2, C2 = 0.03^2; sigma_x^2 = E[x^2] - mu_x^2 ...) and the L1 term, forward and backward.
 * x, y: fp32 logical [B, C, H, W] with element strides {b, c, h, w} (HOST arrays of 4; any layout, NHWC views included),
 * B * C * H * W < 2^31, B <= 65535.  padding: GS_SSIM_SAME averages the SSIM map over every position, GS_SSIM_VALID over
 * [5, H-5) x [5, W-5) (H > 10 and W > 10).  The L1 term is always the mean of |x - y| over every element.
 * work: caller-owned device memory, 16-byte aligned, of gs_ssim_work_bytes(B, C, H, W, train) bytes: the per-block partial
 * sums and, with train, the three coefficient maps the backward reads (3 * B * C * H * W floats).
 * gs_ssim_fwd: one pass over x and y, then a one-block reduction in a fixed order (no atomics: bit-identical from run to run,
 * and between layouts of the same values).  Writes, to the non-null DEVICE pointers among them, out_ssim = mean SSIM,
 * out_l1 = mean |x - y| and out_loss = out_l1 * (1 - ssim_lambda) + (1 - out_ssim) * ssim_lambda.
 * gs_ssim_bwd: dx (its own strides) = w_ssim * grad_ssim[0] * d(mean SSIM)/dx + w_l1 * grad_l1[0] * sign(x - y) / (B C H W),
 * grad_ssim / grad_l1 DEVICE scalars (null allowed where the weight is 0); work is that of a train forward of the same x, y.
 * Neither function synchronises with the host.  gs_ssim_window writes the 11 window weights (float32 roundings of
 * exp(-(i-5)^2 / 4.5) / sum) to a HOST array of n and returns 11. */
#define GS_SSIM_SAME 0
#define GS_SSIM_VALID 1
uint32_t gs_ssim_window(float *out, uint32_t n);
uint64_t gs_ssim_work_bytes(uint32_t B, uint32_t C, uint32_t H, uint32_t W, int32_t train);
int32_t gs_ssim_fwd(const float *x, const int64_t *x_strides, const float *y, const int64_t *y_strides, uint32_t B, uint32_t C,
                    uint32_t H, uint32_t W, int32_t padding, int32_t train, float ssim_lambda, void *work, uint64_t work_bytes,
                    float *out_ssim, float *out_l1, float *out_loss, gs_stream_t stream);
int32_t gs_ssim_bwd(const float *x, const int64_t *x_strides, const float *y, const int64_t *y_strides, uint32_t B, uint32_t C,
                    uint32_t H, uint32_t W, int32_t padding, const void *work, uint64_t work_bytes, const float *grad_ssim,
                    float w_ssim, const float *grad_l1, float w_l1, float *dx, const int64_t *dx_strides, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * B1  The trainers' bilateral-grid colour correction (examples/lib_bilagrid.py: slice, BilateralGrid.forward,
 * total_variation_loss), forward and backward.  No host synchronisation.
 * grids: fp32 [N, 12, L, H, W] contiguous (12 L H W < 2^31).  Points: a logical [B, D1, D2] array (B D1 D2 < 2^31): an image
 * batch [B, Himg, Wimg], rays [B, 1, P] or [B, 1, 1].  rgb: fp32 read through rgb_strides = element strides {b, i, j, channel}
 * (HOST array of 4; columns 0-2 of a 4-channel render work without a copy).  xy: fp32 read through xy_strides in the same
 * way (a b stride of 0 broadcasts one coordinate image), values in [0, 1]; NULL: the pixel centres x = (j + 0.5) / D2,
 * y = (i + 0.5) / D1.  grid_idx: DEVICE int64, entry b reads grid grid_idx[b * idx_stride] clamped to [0, N - 1]; NULL: grid
 * min(b, N - 1).
 * Per point: z = 2 (0.299 r + 0.587 g + 0.114 b) - 1, x, y <- 2 (xy - 0.5); F.grid_sample's align_corners=True,
 * padding_mode="border" trilinear interpolation ((c + 1) / 2 (size - 1) clamped to [0, size - 1]) of 12 values A, a row-major
 * 3x4 matrix; rgb_out = A[:, :3] rgb + A[:, 3].
 * gs_bilagrid_slice_fwd writes out_rgb [B, D1, D2, 3] and / or out_affine [B, D1, D2, 12] (16-byte aligned), contiguous.
 * gs_bilagrid_slice_bwd: from v_out_rgb [B, D1, D2, 3] and / or v_out_affine [B, D1, D2, 12] (contiguous; NULL: zero) writes
 * v_rgb [B, D1, D2, 3] (contiguous; the guidance term is 0 where z was clamped, as torch's) and v_grids [N, 12, L, H, W], which
 * it clears first; either may be NULL.  xy gets no gradient.  The grid gradient is summed per workgroup in LDS and added once
 * per workgroup with float atomics: v_grids can differ in its last bits from run to run, v_rgb cannot.
 * gs_bilagrid_tv_fwd: out[0] (DEVICE) = total_variation_loss(x) for fp32 x [N, C, L, H, W] contiguous (N C L H W < 2^31):
 * (1 / N) sum over the axes L, H, W of sum (x[i+1] - x[i])^2 / max(elements per batch entry of the differenced tensor, 1); an
 * axis of size 1 contributes 0.  Summed in double in a fixed order: bit-identical from run to run.  work: caller-owned device
 * memory, 8-byte aligned, of gs_bilagrid_tv_work_bytes() bytes.  gs_bilagrid_tv_bwd: v_x = grad[0] * d out / d x (grad a
 * DEVICE scalar), a gather over the <= 6 neighbours of each element. */
int32_t gs_bilagrid_slice_fwd(const float *grids, uint32_t N, uint32_t L, uint32_t H, uint32_t W, uint32_t B, uint32_t D1,
                              uint32_t D2, const float *xy, const int64_t *xy_strides, const float *rgb, const int64_t *rgb_strides,
                              const int64_t *grid_idx, int64_t idx_stride, float *out_rgb, float *out_affine, gs_stream_t stream);
int32_t gs_bilagrid_slice_bwd(const float *grids, uint32_t N, uint32_t L, uint32_t H, uint32_t W, uint32_t B, uint32_t D1,
                              uint32_t D2, const float *xy, const int64_t *xy_strides, const float *rgb, const int64_t *rgb_strides,
                              const int64_t *grid_idx, int64_t idx_stride, const float *v_out_rgb, const float *v_out_affine,
                              float *v_grids, float *v_rgb, gs_stream_t stream);
uint64_t gs_bilagrid_tv_work_bytes(void);
int32_t gs_bilagrid_tv_fwd(const float *x, uint32_t N, uint32_t C, uint32_t L, uint32_t H, uint32_t W, void *work,
                           uint64_t work_bytes, float *out, gs_stream_t stream);
int32_t gs_bilagrid_tv_bwd(const float *x, uint32_t N, uint32_t C, uint32_t L, uint32_t H, uint32_t W, const float *grad,
                           float *v_x, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * B1c  The evaluation-time colour matching of the same file (examples/lib_bilagrid.py:56-126, color_correct): masked least squares
 * of a quadratic colour warp, iterated.  No host synchronisation, no atomics: bit-identical from run to run.
 * Pixels: G groups of P pixels of n = 1..3 channels (G P <= 2^31 - 1); every group is one least-squares problem per channel.
 * Features of a pixel x, in double, K = n (n + 1) / 2 + n + 1 columns (3, 6, 10): x_c x_c' for c' >= c (c outer), then x, then 1.
 * A record is the upper triangle of A^T A by rows (K (K + 1) / 2 doubles) followed by A^T b (K doubles):
 * gs_color_correct_record_doubles(n) = 9, 27, 65 (0 for another n).  A warp is K n doubles, w[k n + c].
 *
 * gs_color_correct_pass, one pass over the pixels, does either or both of
 *   apply       (warp != NULL; needs out): out = float(clip(A(x) w, 0, 1)), the product summed in double in column order;
 *   accumulate  (partials != NULL): with y = out where applied and x otherwise, the rows of channel c are those with
 *               lo <= z <= hi (compared in float) for z = x0[c], y[c] and ref[c]; they add A(y)^T A(y) and A(y)^T ref[c] to the
 *               lane's record of channel c, which is reduced over the wave, then over the workgroup: ONE record per workgroup,
 *               partials[((g n + c) blocks + b) record_doubles], every one written (zeros where a workgroup saw no row).
 * x and x0 (the image the mask of the first iteration is taken from) are read at pixel strides x_stride and x0_stride
 * (elements, >= n: columns 0..n-1 of a wider render work without a copy); ref [G P, n] and out [G P, n] are contiguous, and out
 * must not overlap x.  blocks >= 1 workgroups per (group, channel) walk the pixels of a group in a grid-stride loop
 * (blocks n G <= 2^31 - 1; blocks <= 65535).  warp: DEVICE [G, K n] doubles; partials: DEVICE, 8-byte aligned.
 *
 * gs_color_correct_solve: per (group, channel) sums the `blocks` records in a fixed order and solves the K x K normal equations
 * in double through a symmetric eigen-decomposition (cyclic Jacobi): w = V diag(1 / lambda_i if lambda_i > 2^-L max lambda,
 * else 0) V^T A^T b with L = gs_color_correct_rcond_log2() = 40, so a full-rank system gets the least-squares solution and a
 * rank-deficient one (no row, a constant channel, fewer rows than columns) the minimum-norm one; a system with a non-finite sum
 * gets w = 0.  The warp is always finite. */
uint32_t gs_color_correct_rcond_log2(void);
uint32_t gs_color_correct_record_doubles(uint32_t n);
int32_t gs_color_correct_pass(const float *x, int64_t x_stride, const float *x0, int64_t x0_stride, const float *ref, uint32_t G,
                              uint64_t P, uint32_t n, float lo, float hi, const double *warp, float *out, double *partials,
                              uint32_t blocks, gs_stream_t stream);
int32_t gs_color_correct_solve(const double *partials, uint32_t G, uint32_t n, uint32_t blocks, double *warp, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * B2  The spacetime trainer's colour decoder (examples/helper/STG/helper_model.py: Sandwich / getcolormodel(), applied to the
 * 9-channel render at examples/simple_trainer_STG.py:578-581), forward and backward.  No host synchronisation.
 * Per pixel, f[0..8] the rendered feature and r[0..5] the ray: x = (f[3..8], r[0..5]); h[j] = max(0, sum_k w1[12 j + k] x[k]),
 * j = 0..5; out[c] = sigmoid(f[c] + sum_j w2[6 c + j] h[j]), c = 0..2.  w1: fp32 [6, 12] (mlp1.weight), w2: fp32 [3, 6]
 * (mlp2.weight), contiguous DEVICE arrays.
 * features: fp32 [C, H, W, .] with channel stride 1 and ONE pixel stride pix_stride >= 9 (in elements) over the whole [C H W]
 * run: pixel p's channels start at features + p * pix_stride (columns 0-8 of a 10-channel render work without a copy).
 * rays: fp32 [C, 6, H, W], every H x W plane contiguous; plane (c, k) starts at rays + c * ray_cam_stride + k * ray_ch_stride
 * (elements).  C H W < 2^32.  max_blocks: cap of the grid (workgroups of 256 lanes, grid-stride loop); 0 = the library's default.
 * gs_stg_decode_fwd writes out [C, H, W, 3], contiguous.
 * gs_stg_decode_bwd: from v_out [C, H, W, 3] (contiguous) writes v_features [C, H, W, 9] (contiguous) and / or partials
 * [G, 90], G = gs_stg_decode_partial_rows(C, H, W, max_blocks): row b holds workgroup b's sums of v_w1 [6, 12] followed by v_w2
 * [3, 6]; the caller adds the G rows.  Either may be NULL (not needed).  h and out are recomputed.  No float atomics: for one
 * shape and max_blocks the partials are bit-identical from run to run.  The rays get no gradient. */
uint32_t gs_stg_decode_partial_rows(uint32_t C, uint32_t H, uint32_t W, uint32_t max_blocks);
int32_t gs_stg_decode_fwd(uint32_t C, uint32_t H, uint32_t W, const float *features, int64_t pix_stride, const float *rays,
                          int64_t ray_cam_stride, int64_t ray_ch_stride, const float *w1, const float *w2, uint32_t max_blocks,
                          float *out, gs_stream_t stream);
int32_t gs_stg_decode_bwd(uint32_t C, uint32_t H, uint32_t W, const float *features, int64_t pix_stride, const float *rays,
                          int64_t ray_cam_stride, int64_t ray_ch_stride, const float *w1, const float *w2, const float *v_out,
                          uint32_t max_blocks, float *v_features, float *partials, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * The static trainer's appearance module (--app_opt; reference examples/utils.py: AppearanceOptModule, called at
 * examples/simple_trainer.py:766-774), csrc/appearance.hip.  Per camera c and splat n, with a hidden width of 64:
 *   x = cat(embeds[c] [E], features[n] [F], bases(d / max(|d|, 1e-12)) [K]);  d = dirs[c, n], or means[n] - cam_centers[c] when dirs
 *   is NULL;  the first num_bases = (sh_degree + 1)^2 <= K bases are Sloan's fast evaluation, the rest zero;
 *   colors[c, n] = w3 relu(w2 relu(w1 x + b1) + b2) + b3 (+ base[n] when base is given), through a sigmoid when activate != 0.
 * fp32, contiguous: features [N, F], embeds [C, E] (already gathered; NULL or E == 0: a zero embedding), dirs [C, N, 3], means [N, 3],
 * cam_centers [C, 3], w1 [64, E + F + K], b1 [64], w2 [64, 64], b2 [64], w3 [3, 64], b3 [3] (torch's [out, in] layout), base [N, 3]
 * or NULL, colors [C, N, 3].  1 <= F <= 96, 1 <= K <= 25, E + F + K <= 128.  max_blocks: cap of the grid (0 or anything above it = the library's default:
 * two workgroups per CU forward, one backward).
 * gs_appearance_bwd recomputes the activations from the same inputs and, from v_colors [C, N, 3], writes v_features [N, F], v_dirs
 * [C, N, 3] (with dirs) or v_means [N, 3] (with means), v_base [N, 3] -- each may be NULL; the [N, .] ones are summed over the cameras
 * inside the kernel -- and partials [R, L], R = gs_appearance_partial_rows(N, F, E, K, max_blocks), L =
 * gs_appearance_partial_cols(C, F, K): row r holds one wave's sums of v_w1[:, E:] [64, F + K], v_w2 [64, 64], v_w3 [3, 64], v_b2
 * [64], v_b3 [3], one float of padding, and d_pre [C, 64], the gradient of the per-camera pre-activation w1[:, :E] embeds[c] + b1.
 * The caller adds the R rows; then v_b1 = sum_c d_pre[c], v_w1[:, :E] = d_pre^T embeds and v_embeds = d_pre w1[:, :E].  No float
 * atomics: for one shape and max_blocks every output is bit-identical from run to run.  A direction of exactly zero has a finite
 * forward value; its gradient is unspecified. */
uint32_t gs_appearance_partial_rows(uint32_t N, uint32_t F, uint32_t E, uint32_t K, uint32_t max_blocks);
uint64_t gs_appearance_partial_cols(uint32_t C, uint32_t F, uint32_t K);
int32_t gs_appearance_fwd(uint32_t N, uint32_t C, uint32_t F, uint32_t E, uint32_t K, uint32_t num_bases, const float *features,
                          const float *embeds, const float *dirs, const float *means, const float *cam_centers, const float *w1,
                          const float *b1, const float *w2, const float *b2, const float *w3, const float *b3, const float *base,
                          int32_t activate, uint32_t max_blocks, float *colors, gs_stream_t stream);
int32_t gs_appearance_bwd(uint32_t N, uint32_t C, uint32_t F, uint32_t E, uint32_t K, uint32_t num_bases, const float *features,
                          const float *embeds, const float *dirs, const float *means, const float *cam_centers, const float *w1,
                          const float *b1, const float *w2, const float *b2, const float *w3, const float *b3, const float *base,
                          int32_t activate, const float *v_colors, uint32_t max_blocks, float *v_features, float *v_dirs,
                          float *v_means, float *v_base, float *partials, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * D1  The densification strategies (gsplat/strategy/default.py, mcmc.py, ops.py; gsplat/relocation.py).  One thread per
 * gaussian (or per packed row), fp32 arrays, contiguous unless a stride is given, no host synchronisation; N == 0 (and, for the
 * packed statistics, nnz == 0) is a no-op that returns success.
 * gs_relocation: equation 9 of "3D Gaussian Splatting as Markov Chain Monte Carlo" (csrc/compute_relocation.cu:6-38).
 *   opacities [N], scales [N,3], ratios int32 [N] with values in [1, n_max] (values outside are clamped by the kernel),
 *   binoms [n_max, n_max] (binoms[n, k] = C(n, k)), n_max >= 1 -> new_opacities [N], new_scales [N,3]:
 *   x = 1 - (1 - o)^(1/n); new_scale = scale * o / sum_{i=1..n} sum_{k<i} binoms[i-1, k] (-1)^k / sqrt(k+1) * x^(k+1).
 *   Evaluated in double (x through expm1 / log1p, running powers, the sum by columns of binoms) and rounded once to float.
 * gs_inject_noise: the per-step perturbation of the MCMC strategy (ops.py:360-385) from the RAW parameters, in place:
 *   means[n] += Sigma_n * (noise[n] * g(1 - sigmoid(opacities[n])) * scaler), g(x) = 1 / (1 + exp(-100 (x - 0.995))),
 *   Sigma = R diag(exp(scales))^2 R^T, R the rotation of quats[n] (wxyz, normalised as gs_quat_scale_to_covar_preci_fwd does).
 *   means, scales (logs), noise [N,3]; quats [N,4]; opacities (logits) [N].  No [N,3,3] temporary.
 * gs_densify_stats: the running statistics of DefaultStrategy (default.py:203-261).  grad: rows of 2 floats, grad_row_stride
 *   floats apart (2: contiguous; 16: the means2d columns of the compositing backward's gradient rows), scaled by sx, sy.
 *   gaussian_ids == NULL (unpacked): grad [C,N] rows, radii int32 [C,N]; for every camera c with radii[c,n] > 0, in ascending c:
 *     grad2d[n] += hypot(gx * sx, gy * sy); count[n] += 1; radii_state[n] = max(radii_state[n], radii[c,n] / extent).
 *     One thread per gaussian, no atomics: bit-identical from run to run.  nnz is not read.
 *   gaussian_ids int64 [nnz] (packed): grad [nnz] rows, radii int32 [nnz]; the same per row with radii > 0 and an id < N, through
 *     float atomic adds and an integer atomic max on the bit pattern of the non-negative radii_state.  C >= 1 is still required.
 *   radii_state may be NULL.  With several cameras radii_state is the TRUE maximum (the reference's indexed assignment keeps
 *   whichever duplicate index the scatter writes last; for C == 1 the two agree).
 * gs_stg_omega_mask: STG_Strategy._zero_omegabymotion (STG_Strategy.py:326-359) from the RAW parameters.  motion: rows of
 *   motion_row_stride >= 3 floats, the first three read; scales (logs) [N,3]; opacities (logits) [N]; omega [N,4].
 *   mask[n] (one byte, 0 / 1) = |m0| + |m1| + |m2| > motion_min && scale_min < max_k exp(scales[n,k]) < scale_max &&
 *   1 / (1 + exp(-opacities[n])) > opacity_min (the reference's constants: 0.3, 0.2, 0.6, 0.7); omega_new[n,:] = omega[n,:] * mask[n].
 *   IEEE operations in torch's order, no fma contraction.  omega_new is a different array than omega.
 * gs_stg_freeze_grads: the per-step freeze (STG_Strategy.py:105-110, 131-136), in place: omega_grad[n,:] *= mask[n] and
 *   quats_grad[n,:] *= !mask[n], both [N,4]; a multiplication by 0.0f / 1.0f (a non-finite gradient under a zero stays
 *   non-finite, as in grad * mask).  16-byte rows when both arrays are 16-byte aligned. */
int32_t gs_relocation(uint32_t N, const float *opacities, const float *scales, const int32_t *ratios, const float *binoms,
                      uint32_t n_max, float *new_opacities, float *new_scales, gs_stream_t stream);
int32_t gs_inject_noise(uint32_t N, float *means, const float *quats, const float *scales, const float *opacities,
                        const float *noise, float scaler, gs_stream_t stream);
int32_t gs_densify_stats(uint32_t C, uint32_t N, uint64_t nnz, const float *grad, uint64_t grad_row_stride, const int32_t *radii,
                         const int64_t *gaussian_ids, float sx, float sy, float extent, float *grad2d, float *count,
                         float *radii_state, gs_stream_t stream);
int32_t gs_stg_omega_mask(uint32_t N, const float *motion, uint64_t motion_row_stride, const float *scales, const float *opacities,
                          const float *omega, float motion_min, float scale_min, float scale_max, float opacity_min, uint8_t *mask,
                          float *omega_new, gs_stream_t stream);
int32_t gs_stg_freeze_grads(uint32_t N, const uint8_t *mask, float *omega_grad, float *quats_grad, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * Native step driver (round 4): the launches of one rasterization() forward of the common training case --
 * unpacked batch, quats + scales or covars, shared SH coefficients (contiguous or split) or [N,3] colours, three render
 * channels, fixed camera poses -- issued from ONE descriptor in two calls instead of seven operator calls from the host
 * language (the backward goes through gs_rasterize_bwd and gs_projection_rows_bwd / _dyn_bwd directly).  Every launch goes through the operator entry points above: identical results; the operators stay the drop-in
 * boundary, this is the executor around them (the counterpart of gsplat/rendering.py:28-582's orchestration).
 *   gs_step_fwd_begin   gs_projection_rows_fwd (gs_projection_rows_dyn_fwd with dyn_motion) -> [gs_presort_split] -> gs_isect_count_keys -> gs_presort_buckets |
 *                       gs_sort_pairs_u64_i32_drop [-> gs_cumsum_i32 when group_prefix is given]
 *   (the caller waits until every entry of block_sums -- pinned host memory it pre-set to -1 -- is >= 0, sets n_isects /
 *    n_kept_host to the sums of its even / odd entries, sizes the phase-2 buffers with gs_isect_finish_work_bytes /
 *    gs_rasterize_plan and allocates them)
 *   gs_step_fwd_finish  gs_isect_finish_presorted -> gs_rasterize_fwd (zero-filling zero_fill as its side job)
 * With rows_ready the first call starts at gs_isect_count_keys (binning + compositing of rows some other producer wrote).
 * All pointers are device pointers except block_sums (pinned host).  Buffers: radii i32 [C,N], depths [C,N], rows [C,N,16]
 * (64-byte aligned), tiles_per_gauss i32 [C,N], depth_keys i64 [C N], depth_vals i32 [C N] (radix pre-sort only), sort_temp
 * (gs_presort_temp_bytes / gs_sort_temp_bytes of C N), splitters i64 [256] (bucketed), sorted_keys i64 [C N] (radix), perm
 * i32 [C N], n_kept u32 [1], group_sums u32 [ceil(C N / 2^gs_isect_emit_group_shift())], group_prefix i64 of the same length
 * + cumsum_scratch (both or neither), block_sums i32 [C * gs_projection_rows_blocks(N)][2] ([gs_isect_count_blocks(C N)][2] with rows_ready); isect_ids i64 / flatten_ids i32
 * [n_isects], offsets i32 [C, tile_height, tile_width], work (gs_isect_finish_work_bytes), render_colors [C,H,W,3],
 * render_alphas [C,H,W,1], last_ids i32 [C,H,W], scratch (plan.scratch_bytes; NULL: no checkpoints), zero_fill: the gradient rows
 * [C N,16] (+ whatever else the caller wants zeroed behind them). */
typedef struct gs_step {
    uint32_t C, N;
    const float *means, *covars, *quats, *scales, *viewmats, *Ks, *opacities, *colors, *sh_coeffs, *sh_rest;
    uint32_t sh_K, sh_degree;
    int32_t width, height;
    float eps2d, near_plane, far_plane, radius_clip;
    int32_t camera_model, antialiased;
    uint32_t tile_size, tile_width, tile_height;
    int32_t bucketed; /* != 0: the bucketed depth pre-sort where gs_presort_applicable(C N) */
    uint32_t lds_capacity;
    int32_t sh_mask_binary;
    const float *sh_mask_logits; /* the shN mask fused into the SH evaluation (split rows), or NULL */
    float sh_mask_temperature;
    uint32_t rows_ready; /* != 0: rows / radii / depths are inputs (e.g. received through the gaussian-sharded exchange): no projection,
                          * gs_isect_count_keys counts the tiles; block_sums then has gs_isect_count_blocks(C N) entries */
    const float *backgrounds; /* [C,3] or NULL */
    /* phase 1 */
    int32_t *radii;
    float *depths, *rows;
    int32_t *tiles_per_gauss;
    int64_t *depth_keys;
    int32_t *depth_vals;
    void *sort_temp;
    uint64_t sort_temp_bytes;
    int64_t *splitters, *sorted_keys;
    int32_t *perm;
    uint32_t *n_kept, *group_sums;
    int64_t *group_prefix;
    void *cumsum_scratch;
    uint64_t cumsum_scratch_bytes;
    int32_t *block_sums;
    /* phase 2 */
    uint64_t n_isects;
    uint32_t n_kept_host; /* elements the pre-sort kept (sum of the odd entries of block_sums); 0: unknown (no packed pairs) */
    uint32_t reserved1;
    int64_t *isect_ids;
    int32_t *flatten_ids, *offsets;
    void *work;
    uint64_t work_bytes;
    float *render_colors, *render_alphas;
    int32_t *last_ids;
    gs_raster_plan plan;
    void *scratch, *zero_fill;
    uint64_t zero_fill_bytes;
    int32_t finish_phase; /* gs_step_fwd_finish: 0 = binning + compositing, 1 = binning only, 2 = compositing only */
    /* dynamic splats (round 6): dyn_motion != NULL routes the projection through gs_projection_rows_dyn_fwd / _bwd (no SH, no covars;
     * quats / scales / opacities / colors are then written when dyn_quant_mask clamps a parameter) */
    const float *dyn_motion, *dyn_omega, *dyn_trbf_center, *dyn_trbf_scale;
    float dyn_timestamp;
    uint32_t dyn_raw_params, dyn_quant_mask;
    float dyn_min_trbf; /* < 0: no temporal culling */
    float dyn_quant_lo[4], dyn_quant_hi[4], dyn_quant_range[4], dyn_quant_step_norm[4];
    uint8_t *dyn_trbf_alive; /* [N] or NULL */
} gs_step;
/* Layout guard for bindings that mirror the host structs by hand (ctypes, cgo, JNA ...): writes up to n entries --
 * sizeof(struct), then offsetof of the listed fields in this order -- and returns how many the list has.
 *   gs_step:       C, sh_K, eps2d, tile_size, sh_mask_logits, rows_ready, backgrounds, radii, sort_temp_bytes, block_sums, n_isects,
 *                  n_kept_host, work_bytes, plan, scratch, zero_fill_bytes, finish_phase, dyn_motion, dyn_timestamp, dyn_quant_lo,
 *                  dyn_trbf_alive
 *   gs_quant_desc: n, x, out, v_out, v_x, lo, q_step, activation, philox_offset */
uint32_t gs_step_layout(uint64_t *out, uint32_t n);
uint32_t gs_quant_desc_layout(uint64_t *out, uint32_t n);
int32_t gs_step_fwd_begin(gs_step *step, gs_stream_t stream);
int32_t gs_step_fwd_finish(gs_step *step, gs_stream_t stream);

/* ------------------------------------------------------------------------
 * 2D Gaussian splatting (surfels): the operators behind rasterization_2dgs (reference gsplat/rendering.py:1002-1321,
 * csrc/fully_fused_projection_2dgs_*.cu, csrc/rasterize_to_pixels_2dgs_*.cu).  Unpacked layout only: a splat is the flat
 * index c * N + n.  fp32, contiguous, no host synchronisation; C == 0 or N == 0 is a no-op that returns success.
 *
 * gs_projection_2dgs_fwd: per (camera, splat) the ray transform M = K [R q_x s_x | R q_y s_y | mean_c] (row-major 3x3: rows
 *   M_u, M_v, M_w), its screen-space centre and radius, the depth mean_c.z and the camera-space normal (third column of
 *   R rot(q), flipped to face the camera).  Culled splats (z outside [near, far], M_w,x^2 + M_w,y^2 - M_w,z^2 == 0,
 *   radius <= radius_clip, box outside the image) get radii = 0 and zeros in the other outputs.  eps2d is accepted and
 *   unused, as in the reference.
 * gs_projection_2dgs_bwd: ADDS into v_means [N,3], v_quats [N,4], v_scales [N,3] (component 2 is never touched) and, when
 *   given, v_viewmats [C,4,4] (rows 0..2; summed per wave, one atomic per wave and value): the caller zeroes them.  Any of
 *   v_means2d / v_depths / v_normals / v_ray_transforms may be NULL (no gradient arrived); no gradient for Ks.
 *
 * gs_rasterize_2dgs_fwd: one 256-lane workgroup per 16x16 tile composites its list front to back (channels in 1..4; the LAST
 *   colour channel is what distortion and median depth read).  Per (pixel, splat): h_u = px M_w - M_u, h_v = py M_w - M_v,
 *   zeta = h_u x h_v (skipped when zeta_z == 0), s = zeta_xy / zeta_z, weight = min(s.s, 2 |mean2d - p|^2),
 *   alpha = min(0.999, o exp(-weight / 2)); alpha < 1/255 is skipped; the pixel stops before the splat that would bring
 *   T (1 - alpha) <= 1e-4.  Outputs: colours + T background, alphas, camera-space normals, the distortion
 *   sum 2 (w d (1 - T) - w sum_prev w d) (zeros unless distloss), the median depth (last channel of the last contributing
 *   splat reached with T > 0.5; 0 when there is none), and last_ids / median_ids i32 [C,H,W] (indices into flatten_ids, -1:
 *   none) for the backward.  masks (uint8 [C, tile_height, tile_width], optional): tiles with 0 get the background and zeros.
 * gs_rasterize_2dgs_bwd: walks each tile back to front from its last_ids and ADDS (one atomic per wave and value, from waves
 *   with a contributing lane) into v_means2d [C N,2], v_means2d_abs (optional), v_ray_transforms [C N,9], v_colors
 *   [C N,channels], v_opacities [C N], v_normals [C N,3]: the caller zeroes them.  Geometry and opacity get nothing where
 *   o exp(-weight / 2) > 0.999.  v_render_distort is read only with distloss; NULL v_render_* mean zero. */
int32_t gs_projection_2dgs_fwd(uint32_t C, uint32_t N, const float *means, const float *quats, const float *scales,
                               const float *viewmats, const float *Ks, int32_t width, int32_t height, float eps2d,
                               float near_plane, float far_plane, float radius_clip, int32_t *radii, float *means2d,
                               float *depths, float *ray_transforms, float *normals, gs_stream_t stream);
int32_t gs_projection_2dgs_bwd(uint32_t C, uint32_t N, const float *means, const float *quats, const float *scales,
                               const float *viewmats, const float *Ks, const int32_t *radii, const float *ray_transforms,
                               const float *v_means2d, const float *v_depths, const float *v_normals,
                               const float *v_ray_transforms, float *v_means, float *v_quats, float *v_scales,
                               float *v_viewmats, gs_stream_t stream);
int32_t gs_rasterize_2dgs_fwd(uint32_t C, uint32_t N, uint32_t n_isects, uint32_t channels, const float *means2d,
                              const float *ray_transforms, const float *colors, const float *opacities, const float *normals,
                              const float *backgrounds, const uint8_t *masks, uint32_t width, uint32_t height,
                              uint32_t tile_size, uint32_t tile_width, uint32_t tile_height, const int32_t *tile_offsets,
                              const int32_t *flatten_ids, int32_t distloss, float *render_colors, float *render_alphas,
                              float *render_normals, float *render_distort, float *render_median, int32_t *last_ids,
                              int32_t *median_ids, gs_stream_t stream);
int32_t gs_rasterize_2dgs_bwd(uint32_t C, uint32_t N, uint32_t n_isects, uint32_t channels, const float *means2d,
                              const float *ray_transforms, const float *colors, const float *opacities, const float *normals,
                              const float *backgrounds, const uint8_t *masks, uint32_t width, uint32_t height,
                              uint32_t tile_size, uint32_t tile_width, uint32_t tile_height, const int32_t *tile_offsets,
                              const int32_t *flatten_ids, int32_t distloss, const float *render_colors,
                              const float *render_alphas, const int32_t *last_ids, const int32_t *median_ids,
                              const float *v_render_colors, const float *v_render_alphas, const float *v_render_normals,
                              const float *v_render_distort, const float *v_render_median, float *v_means2d,
                              float *v_means2d_abs, float *v_ray_transforms, float *v_colors, float *v_opacities,
                              float *v_normals, gs_stream_t stream);
/* Surface normals of a depth map (reference gsplat/utils.py:108-131): points = origin + depth * direction per pixel
 * (direction = camtoworld rotation applied to ((j + 0.5 - cx) / fx, (i + 0.5 - cy) / fy, 1), normalised unless z_depth),
 * normal = normalize((P[i+1,j] - P[i-1,j]) x (P[i,j+1] - P[i,j-1])) with F.normalize's eps 1e-12, zero on the border.
 * depths [B,H,W], camtoworlds [B,4,4], Ks [B,3,3] -> normals [B,H,W,3], every pixel written.  The backward is a gather (each
 * depth reads the <= 4 normals it took part in): v_depths [B,H,W] is overwritten, no atomics. */
int32_t gs_depth_to_normal_fwd(uint32_t B, uint32_t H, uint32_t W, const float *depths, const float *camtoworlds,
                               const float *Ks, int32_t z_depth, float *normals, gs_stream_t stream);
int32_t gs_depth_to_normal_bwd(uint32_t B, uint32_t H, uint32_t W, const float *depths, const float *camtoworlds,
                               const float *Ks, int32_t z_depth, const float *v_normals, float *v_depths, gs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GSPLAT_HIP_H */
