// codec.hip -- decode of the on-disk quantized attribute format straight into the rasterizer's inputs (gfx950).
//
// "The step after the path" of SURVEY.md section 8(f) rank 3: the reference's eval / viewer path reads the compressed planes
// (gsplat/compression/png_compression.py:166-236 decompress, 312-392 _decompress_png*, 487-520 _decompress_kmeans), builds
// fp32 attribute tensors on the HOST (numpy / torch CPU), moves them to the GPU, undoes the log transform of the means
// (png_compression.py:228-230) and then applies the trainer's activations in front of rasterization()
// (examples/simple_trainer.py:779-786: exp on the scales, sigmoid on the opacities, cat(sh0, shN)).  Here the uint8 planes
// go to the GPU as they are and ONE kernel per splat writes means / quats / scales / opacities / sh0 ready for
// rasterization(): dequantize (same arithmetic as gs_grid_dequantize: float64 like the reference's numpy / torch mix),
// inverse log transform sign(y) expm1(|y|), optional quaternion normalisation, exp, sigmoid.  5 + 3 + 4 + 1 + 3 = 16 bytes
// read and 14 floats written per splat: HBM-bound streaming.  The K-means decode of the higher SH bands is a codebook
// gather (labels -> dequantized centroid rows).
#include "gs_common.h"
#include "decode_act_dev.h"

namespace {

struct DecodeArgs {
    const uint8_t *means_lo, *means_hi; // [n,3] each (16-bit grid)
    const uint8_t *scales, *quats, *opacities, *sh0; // [n,3] [n,4] [n] [n,3]
    float mins[14], maxs[14];           // channels: means 0..2 | scales 3..5 | quats 6..9 | opacity 10 | sh0 11..13
    uint32_t shift[5];                  // right shift of the stored byte per attribute (k-bit planes keep the value in the top bits)
    double levels[5];                   // 2^bits - 1 per attribute
    float *means, *scales_out, *quats_out, *opac_out, *sh0_out;
    int32_t normalize_quats, activate;
};

// the reference's decode of one value: q / levels (float64) * (maxs - mins as fp32) + mins, rounded to fp32
GS_DEV float dequant(uint32_t q, double levels, float mn, float mx) {
    const float range = __fsub_rn(mx, mn);
    return (float)((double)q / levels * (double)range + (double)mn);
}

// expm1(a) for a >= 0 rounded as the reference's decode rounds it.  The reference undoes the log transform with torch.expm1 on the
// CPU, whose fp32 kernel is a float-float (two-word) evaluation built from fp32 adds, multiplies and fused multiply-adds only:
// a = q ln2 + s with ln2 split in two words, exp(s) = 1 + s + s^2 (1/2 + s (1/6 + s p(s))) carried as (high, low) pairs, scaled by
// 2^q, minus one, the two words summed last.  Every operation below is that sequence with the same association, so the result is
// the same bit pattern on any IEEE fp32 unit with an fma; the device library's expm1f is a different polynomial and differs from
// it in the last bit for about one value in eight.  (Checked on the host against torch.expm1 over 8e6 values in [0, 80].)
struct F2 { float x, y; };
GS_DEV F2 f2_add(F2 a, float b) { GS_FP_STRICT // two-sum of the high words, the low word rides along
    const float s = a.x + b, v = s - a.x;
    return {s, ((a.x - (s - v)) + (b - v)) + a.y};
}
GS_DEV F2 f2_add(F2 a, F2 b) { GS_FP_STRICT
    const float s = a.x + b.x, v = s - a.x;
    return {s, ((a.x - (s - v)) + (b.x - v)) + (a.y + b.y)};
}
GS_DEV F2 f2_mul(F2 a, float b) { GS_FP_STRICT
    const float s = a.x * b;
    return {s, __fmaf_rn(a.y, b, __fmaf_rn(a.x, b, -s))};
}
GS_DEV F2 f2_mul(F2 a, F2 b) { GS_FP_STRICT
    const float s = a.x * b.x;
    return {s, __fmaf_rn(a.x, b.y, __fmaf_rn(a.y, b.x, __fmaf_rn(a.x, b.x, -s)))};
}
GS_DEV float expm1_ref(float a) { GS_FP_STRICT
    if (!(a <= 88.72283172607421875f)) return a > 0.f ? __builtin_inff() : a; // overflow; NaN stays NaN
    const float q = rintf(a * 1.442695040888963407359924681001892137426645954152985934135449406931f);
    F2 s = f2_add(F2{a, 0.f}, q * -0.693145751953125f);
    s = f2_add(s, q * -1.428606765330187045e-06f);
    float u = +0.1980960224e-3f;
    u = __fmaf_rn(u, s.x, +0.1394256484e-2f);
    u = __fmaf_rn(u, s.x, +0.8333456703e-2f);
    u = __fmaf_rn(u, s.x, +0.4166637361e-1f);
    F2 t = f2_add(f2_mul(s, u), +0.166666659414234244790680580464e+0f);
    t = f2_add(f2_mul(s, t), 0.5f);
    const float sq = s.x * s.x;
    const F2 s2 = {sq, __fmaf_rn(s.x + s.x, s.y, __fmaf_rn(s.x, s.x, -sq))};
    t = f2_add(s, f2_mul(s2, t));
    { // 1 + t
        const float h = 1.f + t.x;
        t = F2{h, ((1.f - h) + t.x) + t.y};
    }
    const int qi = (int)q; // 0 <= q <= 128: two exact power-of-two factors
    const float p1 = __int_as_float(((qi >> 1) + 127) << 23), p2 = __int_as_float((qi - (qi >> 1) + 127) << 23);
    t = F2{t.x * p1 * p2, t.y * p1 * p2};
    t = f2_add(t, -1.f);
    return t.x + t.y;
}

// the inverse log transform sign(y) * expm1(|y|)  (gsplat/utils.py:40-41); sign(+-0) * x = +0, NaN stays NaN
GS_DEV float inv_log(float y) {
    const float m = expm1_ref(fabsf(y));
    return y > 0.f ? m : (y < 0.f ? -m : (y == 0.f ? 0.f : y));
}

__global__ void __launch_bounds__(GS_BLOCK) inverse_log_kernel(uint64_t n, const float *__restrict__ y, float *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * GS_BLOCK;
    for (uint64_t i = (uint64_t)blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += stride) out[i] = inv_log(y[i]);
}

__global__ void __launch_bounds__(GS_BLOCK) decode_splats_kernel(uint64_t n, DecodeArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * GS_BLOCK + threadIdx.x;
    if (i >= n) return;
    // means: 16-bit grid, then the inverse log transform
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t q = ((uint32_t)a.means_hi[i * 3 + c] << 8) + (uint32_t)a.means_lo[i * 3 + c];
        a.means[i * 3 + c] = inv_log(dequant(q, a.levels[0], a.mins[c], a.maxs[c]));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = dequant((uint32_t)a.scales[i * 3 + c] >> a.shift[1], a.levels[1], a.mins[3 + c], a.maxs[3 + c]);
        a.scales_out[i * 3 + c] = a.activate ? decode_act_scale(v) : v;
    }
    float q4[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) q4[c] = dequant((uint32_t)a.quats[i * 4 + c] >> a.shift[2], a.levels[2], a.mins[6 + c], a.maxs[6 + c]);
    if (a.normalize_quats) { // F.normalize(dim=-1): x / max(||x||, 1e-12)
        const float nrm = decode_norm_divisor(decode_sumsq(decode_sumsq(decode_sumsq(q4[0] * q4[0], q4[1]), q4[2]), q4[3]));
#pragma unroll
        for (int c = 0; c < 4; ++c) q4[c] = q4[c] / nrm;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) a.quats_out[i * 4 + c] = q4[c];
    {
        const float v = dequant((uint32_t)a.opacities[i] >> a.shift[3], a.levels[3], a.mins[10], a.maxs[10]);
        a.opac_out[i] = a.activate ? decode_act_opacity(v) : v;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        a.sh0_out[i * 3 + c] = dequant((uint32_t)a.sh0[i * 3 + c] >> a.shift[4], a.levels[4], a.mins[11 + c], a.maxs[11 + c]);
}

// ---------------------------------------------------------------------------------------------------------------------
// Spacetime splats (gsplat/compression/stg_compression.py:124-143 decompress): the eleven attributes of the STG map decoded to
// the RAW parameter dict of render_dynamic -- no activation, no quaternion normalisation, only the inverse log transform of the
// means.  Nothing couples the channels of a splat here, so a workgroup owns DYN_RUN consecutive splats and walks every attribute
// as the flat element range [first * C, last * C): contiguous bytes in, contiguous floats out, lane k of the wave next to lane
// k + 1 in both; channel = element % C picks the bounds.  38 bytes read, 35 floats written per splat.
#define DYN_ATTRS 11
#define DYN_CHANNELS 35
#define DYN_RUN 1024 // splats per workgroup: a multiple of GS_BLOCK, so every lane walks the same count outside the last block

struct DynDecodeArgs {
    const uint8_t *means_lo, *means_hi;   // [n,3] each
    const uint8_t *plane[DYN_ATTRS];      // [n,C] of attribute k >= 1 ([0] unused); motion: the joined [n,9] plane, or image 0
    const uint8_t *motion1, *motion2;     // images 1, 2 of the motion ([n,3] each) when it comes as three, else NULL
    float *out[DYN_ATTRS];
    float mins[DYN_CHANNELS], maxs[DYN_CHANNELS];
    uint32_t shift[DYN_ATTRS];
    double levels[DYN_ATTRS];
};

// tab[c] for a per-lane c < C out of kernel arguments: constant indices only, so the table stays in scalar registers
template <int C> GS_DEV float pick(const float *tab, uint32_t c) {
    float v = tab[0];
#pragma unroll
    for (int k = 1; k < C; ++k) v = c == (uint32_t)k ? tab[k] : v;
    return v;
}

enum { DYN_PLAIN = 0, DYN_MEANS = 1, DYN_MOTION3 = 2 };

// attribute A (C channels, its bounds at channel offset OFF) of the splats [first, first + count)
template <int A, int C, int OFF, int KIND> GS_DEV void decode_dyn_attr(const DynDecodeArgs &a, uint64_t first, uint32_t count) {
    const uint8_t *__restrict__ in = (KIND == DYN_MEANS ? a.means_lo : a.plane[A]) + first * C;
    float *__restrict__ out = a.out[A] + first * C;
    const uint32_t total = count * C; // <= DYN_RUN * 9
    for (uint32_t k = threadIdx.x; k < total; k += GS_BLOCK) {
        const uint32_t c = k % C; // (first * C is a multiple of C)
        uint32_t q;
        if (KIND == DYN_MEANS) q = ((uint32_t)(a.means_hi + first * C)[k] << 8) + (uint32_t)in[k];
        else if (KIND == DYN_MOTION3) {
            const uint32_t s = k / 9, img = c / 3; // image img holds the channels 3 img .. 3 img + 2 of every splat
            const uint8_t *p = img == 0 ? a.plane[A] : (img == 1 ? a.motion1 : a.motion2);
            q = (uint32_t)p[(first + s) * 3 + (c - img * 3)] >> a.shift[A];
        } else q = (uint32_t)in[k] >> a.shift[A];
        const float v = dequant(q, a.levels[A], pick<C>(a.mins + OFF, c), pick<C>(a.maxs + OFF, c));
        out[k] = KIND == DYN_MEANS ? inv_log(v) : v;
    }
}

__global__ void __launch_bounds__(GS_BLOCK) decode_dynamic_splats_kernel(uint64_t n, DynDecodeArgs a) {
    const uint64_t first = (uint64_t)blockIdx.x * DYN_RUN;
    const uint32_t count = (uint32_t)(n - first < (uint64_t)DYN_RUN ? n - first : (uint64_t)DYN_RUN);
    decode_dyn_attr<0, 3, 0, DYN_MEANS>(a, first, count);
    decode_dyn_attr<1, 3, 3, DYN_PLAIN>(a, first, count);  // scales
    decode_dyn_attr<2, 4, 6, DYN_PLAIN>(a, first, count);  // quats
    decode_dyn_attr<3, 1, 10, DYN_PLAIN>(a, first, count); // opacities
    decode_dyn_attr<4, 1, 11, DYN_PLAIN>(a, first, count); // trbf_center
    decode_dyn_attr<5, 1, 12, DYN_PLAIN>(a, first, count); // trbf_scale
    if (a.motion1 != nullptr) decode_dyn_attr<6, 9, 13, DYN_MOTION3>(a, first, count);
    else decode_dyn_attr<6, 9, 13, DYN_PLAIN>(a, first, count);
    decode_dyn_attr<7, 4, 22, DYN_PLAIN>(a, first, count); // omega
    decode_dyn_attr<8, 3, 26, DYN_PLAIN>(a, first, count); // colors
    if (a.plane[9] != nullptr) decode_dyn_attr<9, 3, 29, DYN_PLAIN>(a, first, count);   // features_dir
    if (a.plane[10] != nullptr) decode_dyn_attr<10, 3, 32, DYN_PLAIN>(a, first, count); // features_time
}

// K-means decode (png_compression.py:487-520): out[r, :] = centroids_quant[labels[r], :] / levels * (maxs - mins) + mins,
// one scalar range for the whole codebook; float64 like the reference (numpy division, 0-dim fp32 range and offset).
__global__ void __launch_bounds__(GS_BLOCK) kmeans_decode_kernel(uint64_t total, uint32_t width, const int32_t *__restrict__ labels,
                                                                 const uint8_t *__restrict__ centroids, uint32_t n_centroids, double levels,
                                                                 float mn, float mx, float *__restrict__ out, uint32_t *__restrict__ n_bad) {
    const uint64_t stride = (uint64_t)gridDim.x * GS_BLOCK;
    for (uint64_t e = (uint64_t)blockIdx.x * GS_BLOCK + threadIdx.x; e < total; e += stride) {
        const uint64_t r = e / width;
        const uint32_t c = (uint32_t)(e - r * width);
        // labels come from a file: one outside the codebook (truncated / mismatched shN.npz) must not become a wild read.
        // The reference's centroids[labels] raises IndexError there; here the row decodes to NaN and the count of such
        // labels is reported (n_bad), which the host wrapper turns into the same error.
        const uint32_t lab = (uint32_t)labels[r];
        if (lab >= n_centroids) {
            out[e] = __builtin_nanf("");
            if (c == 0 && n_bad != nullptr) atomicAdd(n_bad, 1u);
            continue;
        }
        out[e] = dequant((uint32_t)centroids[(uint64_t)lab * width + c], levels, mn, mx);
    }
}

} // namespace

extern "C" int32_t gs_decode_splats(
    uint64_t n, const uint8_t *means_lo, const uint8_t *means_hi, const uint8_t *scales, const uint8_t *quats,
    const uint8_t *opacities, const uint8_t *sh0, const float *mins14, const float *maxs14, const uint32_t *bits5,
    int32_t normalize_quats, int32_t activate, float *means_out, float *scales_out, float *quats_out, float *opacities_out,
    float *sh0_out, gs_stream_t stream) {
    if (n == 0) return 0;
    GS_CHECK_ARG(means_lo && means_hi && scales && quats && opacities && sh0 && mins14 && maxs14 && bits5, "null pointer");
    GS_CHECK_ARG(means_out && scales_out && quats_out && opacities_out && sh0_out, "null pointer");
    GS_CHECK_ARG(bits5[0] == 16, "the means are a 16-bit grid");
    DecodeArgs a;
    a.means_lo = means_lo; a.means_hi = means_hi; a.scales = scales; a.quats = quats; a.opacities = opacities; a.sh0 = sh0;
    for (int c = 0; c < 14; ++c) { a.mins[c] = mins14[c]; a.maxs[c] = maxs14[c]; } // HOST arrays (14 floats of meta.json)
    for (int k = 0; k < 5; ++k) {
        GS_CHECK_ARG(k == 0 || (bits5[k] >= 1 && bits5[k] <= 8), "plane bit depths must be in 1..8");
        a.levels[k] = (double)((1u << bits5[k]) - 1u);
        a.shift[k] = k == 0 ? 0u : 8u - bits5[k];
    }
    a.means = means_out; a.scales_out = scales_out; a.quats_out = quats_out; a.opac_out = opacities_out; a.sh0_out = sh0_out;
    a.normalize_quats = normalize_quats; a.activate = activate;
    GS_CHECK_ARG(gs_div_up(n, GS_BLOCK) < (1ull << 31), "too many splats");
    hipLaunchKernelGGL(decode_splats_kernel, dim3((uint32_t)gs_div_up(n, GS_BLOCK)), dim3(GS_BLOCK), 0, (hipStream_t)stream, n, a);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_inverse_log_transform(uint64_t n, const float *y, float *out, gs_stream_t stream) {
    if (n == 0) return 0;
    GS_CHECK_ARG(y && out, "null pointer");
    const uint32_t blocks = (uint32_t)(gs_div_up(n, GS_BLOCK) < 8192u ? gs_div_up(n, GS_BLOCK) : 8192u);
    hipLaunchKernelGGL(inverse_log_kernel, dim3(blocks), dim3(GS_BLOCK), 0, (hipStream_t)stream, n, y, out);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_decode_dynamic_splats(uint64_t n, const uint8_t *const *planes14, const float *mins35, const float *maxs35,
                                            const uint32_t *bits11, float *const *outs11, gs_stream_t stream) {
    if (n == 0) return 0;
    GS_CHECK_ARG(planes14 && mins35 && maxs35 && bits11 && outs11, "null pointer");
    // planes14: means_l means_u scales quats opacities trbf_center trbf_scale motion(0) motion1 motion2 omega colors
    // features_dir features_time; outs11 in the attribute order.  The last two attributes are optional.
    static const int plane_of[DYN_ATTRS] = {0, 2, 3, 4, 5, 6, 7, 10, 11, 12, 13};
    DynDecodeArgs a;
    a.means_lo = planes14[0]; a.means_hi = planes14[1]; a.motion1 = planes14[8]; a.motion2 = planes14[9];
    GS_CHECK_ARG(a.means_lo && a.means_hi, "null pointer (means planes)");
    GS_CHECK_ARG((a.motion1 == nullptr) == (a.motion2 == nullptr), "the motion is one joined plane or three images");
    GS_CHECK_ARG(bits11[0] == 16, "the means are a 16-bit grid");
    for (int k = 0; k < DYN_ATTRS; ++k) {
        a.plane[k] = k == 0 ? nullptr : planes14[plane_of[k]];
        a.out[k] = outs11[k];
        const bool optional = k >= 9;
        GS_CHECK_ARG(optional || ((k == 0 || a.plane[k]) && a.out[k]), "null pointer (required attribute)");
        GS_CHECK_ARG(!optional || a.plane[k] == nullptr || a.out[k] != nullptr, "null output of a present attribute");
        GS_CHECK_ARG(k == 0 || (bits11[k] >= 1 && bits11[k] <= 8), "plane bit depths must be in 1..8");
        a.levels[k] = (double)((1u << bits11[k]) - 1u);
        a.shift[k] = k == 0 ? 0u : 8u - bits11[k];
    }
    for (int c = 0; c < DYN_CHANNELS; ++c) { a.mins[c] = mins35[c]; a.maxs[c] = maxs35[c]; } // HOST arrays (meta.json)
    GS_CHECK_ARG((n + DYN_RUN - 1) / DYN_RUN < (1ull << 31), "too many splats");
    hipLaunchKernelGGL(decode_dynamic_splats_kernel, dim3((uint32_t)((n + DYN_RUN - 1) / DYN_RUN)), dim3(GS_BLOCK), 0,
                       (hipStream_t)stream, n, a);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_kmeans_decode(uint64_t n_rows, uint32_t width, const int32_t *labels, const uint8_t *centroids_quant,
                                    uint32_t n_centroids, uint32_t bits, float mins, float maxs, float *out, uint32_t *n_bad,
                                    gs_stream_t stream) {
    if (n_rows == 0 || width == 0) return 0;
    GS_CHECK_ARG(labels && centroids_quant && out, "null pointer");
    GS_CHECK_ARG(bits >= 1 && bits <= 8, "bits must be in 1..8");
    const uint64_t total = n_rows * width;
    const uint32_t blocks = (uint32_t)(gs_div_up(total, GS_BLOCK) < 16384u ? gs_div_up(total, GS_BLOCK) : 16384u);
    hipLaunchKernelGGL(kmeans_decode_kernel, dim3(blocks), dim3(GS_BLOCK), 0, (hipStream_t)stream, total, width, labels, centroids_quant,
                       n_centroids, (double)((1u << bits) - 1u), mins, maxs, out, n_bad);
    GS_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// PNG scanline reconstruction (host code; the inverse of the five PNG filter types, PNG specification section 9): the
// sequential-in-x part of reading the reference's image grids (imageio / Pillow write them with adaptive filters).
// data: h rows of (1 + stride) bytes -- filter type, then the filtered scanline; out: h rows of stride bytes.
extern "C" int32_t gs_png_unfilter(const uint8_t *data, uint32_t h, uint32_t stride, uint32_t bpp, uint8_t *out) {
    GS_CHECK_ARG(data && out && bpp >= 1 && bpp <= 8 && stride >= bpp, "null pointer / bytes per pixel");
    for (uint32_t y = 0; y < h; ++y) {
        const uint8_t *src = data + (size_t)y * (stride + 1);
        const uint8_t ft = src[0];
        const uint8_t *in = src + 1, *up = y ? out + (size_t)(y - 1) * stride : nullptr;
        uint8_t *o = out + (size_t)y * stride;
        GS_CHECK_ARG(ft <= 4, "unknown PNG filter type");
        for (uint32_t x = 0; x < stride; ++x) {
            const int a = x >= bpp ? o[x - bpp] : 0, b = up ? up[x] : 0, c = (up && x >= bpp) ? up[x - bpp] : 0;
            int pred = 0;
            if (ft == 1) pred = a;
            else if (ft == 2) pred = b;
            else if (ft == 3) pred = (a + b) >> 1;
            else if (ft == 4) {
                const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
                pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
            }
            o[x] = (uint8_t)(in[x] + pred);
        }
    }
    return 0;
}
