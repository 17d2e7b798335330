// stg_decoder.hip -- the spacetime trainer's colour decoder (examples/helper/STG/helper_model.py: Sandwich, what getcolormodel()
// returns; called at examples/simple_trainer_STG.py:578-581 on the 9-channel render), forward and backward
// (gs_stg_decode_fwd / _bwd): a per-pixel, bias-free 12 -> 6 -> 3 MLP with a ReLU between its two 1x1 convolutions, whose output is
// added to the albedo channels before a sigmoid.
//
// Per pixel, f[0..8] the rendered feature, r[0..5] the ray:
//   x      = (f[3..8], r[0..5])                            mlp1's column order: spec, timefeature, rays
//   h[j]   = max(0, sum_k W1[j][k] x[k])                   j = 0..5
//   out[c] = sigmoid(f[c] + sum_j W2[c][j] h[j])           c = 0..2
// Backward, given v_out:
//   g[c] = v_out[c] out[c] (1 - out[c]);  v_f[0..2] = g;  v_h[j] = (h[j] > 0) sum_c W2[c][j] g[c];
//   v_f[3 + k] = sum_j W1[j][k] v_h[j] (k = 0..5);  v_W2[c][j] = sum_pixels g[c] h[j];  v_W1[j][k] = sum_pixels v_h[j] x[k].
//
// Layouts.  Features [C, H, W, .]: channel stride 1, one pixel stride >= 9 in elements for the whole [C H W] run, so columns 0-8 of
// a 10-channel RGB+D render are read in place.  Rays [C, 6, H, W], every H x W plane contiguous, camera and channel strides given:
// coalesced dword loads.  Output [C, H, W, 3] and v_features [C, H, W, 9] contiguous.
//
// Both kernels: one lane per pixel in a grid-stride loop over at most max_blocks workgroups.  The 90 weights sit at wave-uniform
// addresses and are read once per lane, in front of the loop, into registers.  72 B of traffic per pixel forward (36 + 24 in, 12
// out), 108 B backward (36 + 24 + 12 in, 36 out: out is recomputed, not saved), ~200 / ~450 FLOPs: both are streaming kernels.
//
// Weight gradient.  A lane keeps the 90 sums of its pixels in registers; after the loop they are reduced over the wave (DPP,
// dpp_reduce.h: ten groups of nine), over the workgroup's four waves through LDS in a fixed order, and workgroup b stores row b
// of partials [G, 90] (row: v_W1 [6][12], then v_W2 [3][6]).  The caller sums the G rows.  No float atomics: for a given grid the
// result is bit-identical from run to run.
#include "gs_common.h"
#include "dpp_reduce.h"

#define SD_MAX_BLOCKS 2048  // 256 CUs x 8 workgroups
#define SD_W1 72
#define SD_W2 18
#define SD_SUMS (SD_W1 + SD_W2)

namespace {

struct DecodeGeo {
    const float *features;
    int64_t pix_stride;
    const float *rays;
    int64_t ray_cam_stride, ray_ch_stride;
    const float *w1, *w2;
    uint32_t n, hw;  // pixels in all, per camera
};

struct Pixel {
    float f[9], x[12], h[6], out[3];
};

GS_DEV void load_weights(const DecodeGeo &g, float w1[SD_W1], float w2[SD_W2]) {
#pragma unroll
    for (int i = 0; i < SD_W1; ++i) w1[i] = g.w1[i];
#pragma unroll
    for (int i = 0; i < SD_W2; ++i) w2[i] = g.w2[i];
}

// (explicit fmas under GS_FP_STRICT: the forward, the backward's recomputation and its three instantiations round alike, so a half
// of the backward is bit-identical to the same half of the full one)
GS_DEV void decode_pixel(const DecodeGeo &g, uint32_t p, const float w1[SD_W1], const float w2[SD_W2], Pixel &px) {
    GS_FP_STRICT;
    const float *f = g.features + (int64_t)p * g.pix_stride;
    const uint32_t c = p / g.hw, r = p - c * g.hw;
    const float *ray = g.rays + (int64_t)c * g.ray_cam_stride + r;
#pragma unroll
    for (int k = 0; k < 9; ++k) px.f[k] = f[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        px.x[k] = px.f[3 + k];
        px.x[6 + k] = ray[(int64_t)k * g.ray_ch_stride];
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 12; ++k) s = fmaf(w1[12 * j + k], px.x[k], s);
        px.h[j] = fmaxf(s, 0.f);
    }
#pragma unroll
    for (int c3 = 0; c3 < 3; ++c3) {
        float s = px.f[c3];
#pragma unroll
        for (int j = 0; j < 6; ++j) s = fmaf(w2[6 * c3 + j], px.h[j], s);
        px.out[c3] = 1.f / (1.f + expf(-s));
    }
}

__global__ void __launch_bounds__(GS_BLOCK) stg_decode_fwd_kernel(DecodeGeo g, float *__restrict__ out) {
    float w1[SD_W1], w2[SD_W2];
    load_weights(g, w1, w2);
    const uint64_t step = (uint64_t)gridDim.x * GS_BLOCK;
    for (uint64_t p = (uint64_t)blockIdx.x * GS_BLOCK + threadIdx.x; p < g.n; p += step) {
        Pixel px;
        decode_pixel(g, (uint32_t)p, w1, w2, px);
        float *o = out + 3 * p;
        o[0] = px.out[0];
        o[1] = px.out[1];
        o[2] = px.out[2];
    }
}

template <bool WANT_F, bool WANT_W>
__global__ void __launch_bounds__(GS_BLOCK) stg_decode_bwd_kernel(DecodeGeo g, const float *__restrict__ v_out,
                                                                  float *__restrict__ v_features, float *__restrict__ partials) {
    GS_FP_STRICT;
    __shared__ float s_part[GS_BLOCK / GS_WAVE][SD_SUMS];
    float w1[SD_W1], w2[SD_W2];
    load_weights(g, w1, w2);
    float acc[SD_SUMS];
#pragma unroll
    for (int i = 0; i < SD_SUMS; ++i) acc[i] = 0.f;
    const uint64_t step = (uint64_t)gridDim.x * GS_BLOCK;
    for (uint64_t p = (uint64_t)blockIdx.x * GS_BLOCK + threadIdx.x; p < g.n; p += step) {
        Pixel px;
        decode_pixel(g, (uint32_t)p, w1, w2, px);
        const float *vo = v_out + 3 * p;
        float gr[3], vh[6];
#pragma unroll
        for (int c = 0; c < 3; ++c) gr[c] = vo[c] * px.out[c] * (1.f - px.out[c]);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const float s = fmaf(w2[12 + j], gr[2], fmaf(w2[6 + j], gr[1], w2[j] * gr[0]));
            vh[j] = px.h[j] > 0.f ? s : 0.f;
        }
        if (WANT_F) {
            float *vf = v_features + 9 * p;
            vf[0] = gr[0];
            vf[1] = gr[1];
            vf[2] = gr[2];
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < 6; ++j) s = fmaf(w1[12 * j + k], vh[j], s);
                vf[3 + k] = s;
            }
        }
        if (WANT_W) {
#pragma unroll
            for (int j = 0; j < 6; ++j)
#pragma unroll
                for (int k = 0; k < 12; ++k) acc[12 * j + k] = fmaf(vh[j], px.x[k], acc[12 * j + k]);
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 6; ++j) acc[SD_W1 + 6 * c + j] = fmaf(gr[c], px.h[j], acc[SD_W1 + 6 * c + j]);
        }
    }
    if (WANT_W) {
        // (every lane of every wave is here, with zeros where it had no pixel: the DPP sums need the whole wave)
#pragma unroll
        for (int i = 0; i < SD_SUMS; i += 9)
            wave_reduce_sum_9(acc[i], acc[i + 1], acc[i + 2], acc[i + 3], acc[i + 4], acc[i + 5], acc[i + 6], acc[i + 7], acc[i + 8]);
        if (lane_id() == GS_WAVE - 1) {
#pragma unroll
            for (int i = 0; i < SD_SUMS; ++i) s_part[threadIdx.x / GS_WAVE][i] = acc[i];
        }
        __syncthreads();
        if (threadIdx.x < SD_SUMS) {
            float s = s_part[0][threadIdx.x];
#pragma unroll
            for (int w = 1; w < GS_BLOCK / GS_WAVE; ++w) s += s_part[w][threadIdx.x];
            partials[(uint64_t)blockIdx.x * SD_SUMS + threadIdx.x] = s;
        }
    }
}

uint32_t decode_blocks(uint64_t n, uint32_t max_blocks) {
    const uint32_t cap = max_blocks ? max_blocks : SD_MAX_BLOCKS;
    const uint64_t need = (n + GS_BLOCK - 1) / GS_BLOCK;
    return (uint32_t)(need < cap ? (need ? need : 1) : cap);
}

int32_t decode_geo(const char *fn, DecodeGeo &g, uint32_t C, uint32_t H, uint32_t W, const float *features, int64_t pix_stride,
                   const float *rays, int64_t ray_cam_stride, int64_t ray_ch_stride, const float *w1, const float *w2) {
    if (!features || !rays || !w1 || !w2) {
        gs_set_error("%s: null pointer (features, rays, w1 and w2 are required)", fn);
        return 1;
    }
    if (C == 0 || H == 0 || W == 0) {
        gs_set_error("%s: empty shape [%u, %u, %u]", fn, C, H, W);
        return 1;
    }
    if (pix_stride < 9) {
        gs_set_error("%s: a pixel stride of %lld elements, below the 9 channels read", fn, (long long)pix_stride);
        return 1;
    }
    const uint64_t hw = (uint64_t)H * W;
    if (hw > 0xffffffffull || hw * C > 0xffffffffull) {
        gs_set_error("%s: [%u, %u, %u] has more than 2^32 - 1 pixels", fn, C, H, W);
        return 1;
    }
    if (ray_ch_stride < 0 || ray_cam_stride < 0) {
        gs_set_error("%s: negative ray strides (%lld, %lld)", fn, (long long)ray_cam_stride, (long long)ray_ch_stride);
        return 1;
    }
    if ((((uintptr_t)features | (uintptr_t)rays | (uintptr_t)w1 | (uintptr_t)w2) % 4) != 0) {
        gs_set_error("%s: misaligned pointer (floats need 4-byte alignment)", fn);
        return 1;
    }
    g.features = features;
    g.pix_stride = pix_stride;
    g.rays = rays;
    g.ray_cam_stride = ray_cam_stride;
    g.ray_ch_stride = ray_ch_stride;
    g.w1 = w1;
    g.w2 = w2;
    g.hw = (uint32_t)hw;
    g.n = (uint32_t)(hw * C);
    return 0;
}

}  // namespace

extern "C" uint32_t gs_stg_decode_partial_rows(uint32_t C, uint32_t H, uint32_t W, uint32_t max_blocks) {
    return decode_blocks((uint64_t)C * H * W, max_blocks);
}

extern "C" int32_t gs_stg_decode_fwd(uint32_t C, uint32_t H, uint32_t W, const float *features, int64_t pix_stride, const float *rays,
                                     int64_t ray_cam_stride, int64_t ray_ch_stride, const float *w1, const float *w2,
                                     uint32_t max_blocks, float *out, gs_stream_t stream) {
    DecodeGeo g;
    if (decode_geo("gs_stg_decode_fwd", g, C, H, W, features, pix_stride, rays, ray_cam_stride, ray_ch_stride, w1, w2)) return 1;
    GS_CHECK_ARG(out, "null pointer: no output");
    GS_CHECK_ARG((uintptr_t)out % 4 == 0, "out must be 4-byte aligned");
    hipLaunchKernelGGL(stg_decode_fwd_kernel, dim3(decode_blocks(g.n, max_blocks)), dim3(GS_BLOCK), 0, (hipStream_t)stream, g, out);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_stg_decode_bwd(uint32_t C, uint32_t H, uint32_t W, const float *features, int64_t pix_stride, const float *rays,
                                     int64_t ray_cam_stride, int64_t ray_ch_stride, const float *w1, const float *w2,
                                     const float *v_out, uint32_t max_blocks, float *v_features, float *partials,
                                     gs_stream_t stream) {
    DecodeGeo g;
    if (decode_geo("gs_stg_decode_bwd", g, C, H, W, features, pix_stride, rays, ray_cam_stride, ray_ch_stride, w1, w2)) return 1;
    GS_CHECK_ARG(v_out, "null pointer: no upstream gradient");
    GS_CHECK_ARG(v_features || partials, "null pointer: no output (v_features and partials both null)");
    GS_CHECK_ARG(((uintptr_t)v_out | (uintptr_t)v_features | (uintptr_t)partials) % 4 == 0, "the gradient arrays must be 4-byte aligned");
    const dim3 grid(decode_blocks(g.n, max_blocks)), block(GS_BLOCK);
    const hipStream_t st = (hipStream_t)stream;
    if (v_features && partials)
        hipLaunchKernelGGL((stg_decode_bwd_kernel<true, true>), grid, block, 0, st, g, v_out, v_features, partials);
    else if (v_features)
        hipLaunchKernelGGL((stg_decode_bwd_kernel<true, false>), grid, block, 0, st, g, v_out, v_features, partials);
    else
        hipLaunchKernelGGL((stg_decode_bwd_kernel<false, true>), grid, block, 0, st, g, v_out, v_features, partials);
    GS_CHECK_LAUNCH();
    return 0;
}
