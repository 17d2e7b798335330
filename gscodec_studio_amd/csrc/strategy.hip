// strategy.hip -- the kernels of the densification strategies (gsplat/strategy/default.py, mcmc.py, ops.py; gsplat/relocation.py).
//
// gs_densify_stats  DefaultStrategy._update_state: the running image-plane gradient norm, visibility count and screen-space radius
//                   of every gaussian, in one launch instead of clone / scale / nonzero / gather / norm / index_add / scatter.
// gs_inject_noise   MCMCStrategy's per-step perturbation of the means, from the raw parameters, in one launch.
// gs_relocation     equation 9 of the MCMC paper (the opacity and scale of a gaussian that stands for n copies of itself).
// gs_stg_omega_mask   STG_Strategy._zero_omegabymotion: which gaussians keep a trainable omega, and omega with the others zeroed.
// gs_stg_freeze_grads STG_Strategy's per-step freeze: omega.grad *= mask, quats.grad *= !mask, both in place in one launch.
//
// All of them are one thread per gaussian (or per packed row) in GS_BLOCK-thread blocks.  The two per-step kernels are streaming
// kernels; their minimum traffic per gaussian is 12 C + 8 bytes (+ 8 with the radii state) for the unpacked statistics (8 C of
// them the gradient, of which a 64-byte-strided gradient row costs a whole 64-byte sector per camera instead) and 68 bytes for the
// noise (14 floats read, 3 written).  The freeze moves 65 bytes per gaussian (two 16-byte rows read and written, one mask byte), the
// mask build 61 (3 of the motion row's floats -- whole sectors of it in practice --, 3 + 1 + 4 floats read, 4 floats + 1 byte written).
#include "gs_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------------
// gs_densify_stats
// ---------------------------------------------------------------------------------------------------------------------------------
template <bool VEC2>
GS_DEV void load_grad(const float *grad, uint64_t row, uint64_t stride, float &gx, float &gy) {
    const float *p = grad + row * stride;
    if (VEC2) {
        const float2 g = *reinterpret_cast<const float2 *>(p);
        gx = g.x;
        gy = g.y;
    } else {
        gx = p[0];
        gy = p[1];
    }
}

// unpacked: thread n walks the cameras (for each c the wave reads consecutive n); every output element has one writer
template <bool VEC2>
__global__ void __launch_bounds__(GS_BLOCK) densify_stats_kernel(uint32_t C, uint32_t N, const float *__restrict__ grad, uint64_t stride,
                                                                 const int32_t *__restrict__ radii, float sx, float sy, float extent,
                                                                 float *__restrict__ grad2d, float *__restrict__ count,
                                                                 float *__restrict__ radii_state) {
    const uint32_t n = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (n >= N) return;
    float sum = 0.f, seen = 0.f;
    int32_t rmax = 0;
    bool any = false;
    for (uint32_t c = 0; c < C; ++c) {
        const uint64_t e = (uint64_t)c * N + n;
        const int32_t r = radii[e];
        if (r <= 0) continue;
        float gx, gy;
        load_grad<VEC2>(grad, e, stride, gx, gy);
        sum += hypotf(gx * sx, gy * sy);  // ascending c: a fixed order
        seen += 1.f;
        rmax = r > rmax ? r : rmax;
        any = true;
    }
    if (!any) return;
    grad2d[n] += sum;
    count[n] += seen;
    if (radii_state != nullptr) {
        const float v = (float)rmax / extent;
        if (v > radii_state[n]) radii_state[n] = v;
    }
}

// packed: one thread per (camera, gaussian) row; several rows may name the same gaussian
template <bool VEC2>
__global__ void __launch_bounds__(GS_BLOCK) densify_stats_packed_kernel(uint64_t nnz, uint32_t N, const float *__restrict__ grad,
                                                                        uint64_t stride, const int32_t *__restrict__ radii,
                                                                        const int64_t *__restrict__ ids, float sx, float sy,
                                                                        float extent, float *grad2d, float *count, float *radii_state) {
    const uint64_t e = (uint64_t)blockIdx.x * GS_BLOCK + threadIdx.x;
    if (e >= nnz) return;
    const int32_t r = radii[e];
    const int64_t id = ids[e];
    if (r <= 0 || id < 0 || id >= (int64_t)N) return;
    float gx, gy;
    load_grad<VEC2>(grad, e, stride, gx, gy);
    atomicAdd(grad2d + id, hypotf(gx * sx, gy * sy));
    atomicAdd(count + id, 1.f);
    if (radii_state != nullptr) {
        // non-negative floats order like their bit patterns
        const float v = (float)r / extent;
        atomicMax(reinterpret_cast<int32_t *>(radii_state) + id, __float_as_int(v));
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// gs_inject_noise
// ---------------------------------------------------------------------------------------------------------------------------------
template <bool VEC4>
__global__ void __launch_bounds__(GS_BLOCK) inject_noise_kernel(uint32_t N, float *__restrict__ means, const float *__restrict__ quats,
                                                                const float *__restrict__ scales, const float *__restrict__ opacities,
                                                                const float *__restrict__ noise, float scaler) {
    const uint32_t n = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (n >= N) return;
    float qw, qx, qy, qz;
    if (VEC4) {
        const float4 q = reinterpret_cast<const float4 *>(quats)[n];
        qw = q.x; qx = q.y; qy = q.z; qz = q.w;
    } else {
        qw = quats[4ull * n]; qx = quats[4ull * n + 1]; qy = quats[4ull * n + 2]; qz = quats[4ull * n + 3];
    }
    const uint64_t b = 3ull * n;
    const float s0 = expf(scales[b]), s1 = expf(scales[b + 1]), s2 = expf(scales[b + 2]);
    // 1 - sigmoid(l) = 1 / (1 + exp(l)), without the cancellation of the subtraction
    const float x = 1.f / (1.f + expf(opacities[n]));
    const float w = scaler / (1.f + expf(-100.f * (x - 0.995f)));
    const float v0 = noise[b] * w, v1 = noise[b + 1] * w, v2 = noise[b + 2] * w;
    const Mat3 R = quat_to_rotmat(qw, qx, qy, qz);
    // Sigma v = R S^2 R^T v
    const float t0 = (R.m[0][0] * v0 + R.m[1][0] * v1 + R.m[2][0] * v2) * (s0 * s0);
    const float t1 = (R.m[0][1] * v0 + R.m[1][1] * v1 + R.m[2][1] * v2) * (s1 * s1);
    const float t2 = (R.m[0][2] * v0 + R.m[1][2] * v1 + R.m[2][2] * v2) * (s2 * s2);
    means[b] += R.m[0][0] * t0 + R.m[0][1] * t1 + R.m[0][2] * t2;
    means[b + 1] += R.m[1][0] * t0 + R.m[1][1] * t1 + R.m[1][2] * t2;
    means[b + 2] += R.m[2][0] * t0 + R.m[2][1] * t1 + R.m[2][2] * t2;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// gs_relocation
// ---------------------------------------------------------------------------------------------------------------------------------
// The reference sums binoms[i-1, k] (-1)^k / sqrt(k+1) x^(k+1) over i = 1..n, k < i in float with a pow per term.  The terms
// alternate and reach e^(n x) times the sum, and x itself is a difference of numbers near 1, so its float result is off by up to
// a few 1e-4 at large n.  Here the sum is taken by columns -- sum_k (-1)^k x^(k+1) / sqrt(k+1) * (sum_{i>k} binoms[i-1, k]) -- in double:
// the column sums are exact (integers below 2^53), the power runs along k, and x comes from expm1 / log1p.
__global__ void __launch_bounds__(GS_BLOCK) relocation_kernel(uint32_t N, const float *__restrict__ opacities,
                                                              const float *__restrict__ scales, const int32_t *__restrict__ ratios,
                                                              const float *__restrict__ binoms, uint32_t n_max,
                                                              float *__restrict__ new_opacities, float *__restrict__ new_scales) {
    const uint32_t idx = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (idx >= N) return;
    const int32_t r = ratios[idx];
    const uint32_t n = r < 1 ? 1u : ((uint32_t)r > n_max ? n_max : (uint32_t)r);
    const double o = (double)opacities[idx];
    const double x = -expm1(log1p(-o) / (double)n);
    double denom = 0.0, xp = x;
    for (uint32_t k = 0; k < n; ++k) {
        double col = 0.0;
        for (uint32_t i = k + 1; i <= n; ++i) col += (double)binoms[(uint64_t)(i - 1) * n_max + k];
        const double t = col * xp / sqrt((double)(k + 1));
        denom += (k & 1u) ? -t : t;
        xp *= x;
    }
    const double coeff = o / denom;
    new_opacities[idx] = (float)x;
    const uint64_t b = 3ull * idx;
    new_scales[b] = (float)(coeff * (double)scales[b]);
    new_scales[b + 1] = (float)(coeff * (double)scales[b + 1]);
    new_scales[b + 2] = (float)(coeff * (double)scales[b + 2]);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// gs_stg_omega_mask / gs_stg_freeze_grads
// ---------------------------------------------------------------------------------------------------------------------------------
template <bool VEC4>
GS_DEV float4 load_row4(const float *p, uint64_t n) {
    if (VEC4) return reinterpret_cast<const float4 *>(p)[n];
    return make_float4(p[4 * n], p[4 * n + 1], p[4 * n + 2], p[4 * n + 3]);
}

template <bool VEC4>
GS_DEV void store_row4(float *p, uint64_t n, float4 v) {
    if (VEC4) {
        reinterpret_cast<float4 *>(p)[n] = v;
    } else {
        p[4 * n] = v.x; p[4 * n + 1] = v.y; p[4 * n + 2] = v.z; p[4 * n + 3] = v.w;
    }
}

// torch's operations in torch's order, uncontracted: sum(abs(motion[:, 0:3]), 1), max(exp(scales), 1), sigmoid = 1 / (1 + exp(-x))
template <bool VEC4>
__global__ void __launch_bounds__(GS_BLOCK) stg_omega_mask_kernel(uint32_t N, const float *__restrict__ motion, uint64_t motion_stride,
                                                                  const float *__restrict__ scales, const float *__restrict__ opacities,
                                                                  const float *__restrict__ omega, float motion_min, float scale_min,
                                                                  float scale_max, float opacity_min, uint8_t *__restrict__ mask,
                                                                  float *__restrict__ omega_new) {
    GS_FP_STRICT;
    const uint32_t n = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (n >= N) return;
    const float *m = motion + (uint64_t)n * motion_stride;
    const float moved = (fabsf(m[0]) + fabsf(m[1])) + fabsf(m[2]);
    const uint64_t b = 3ull * n;
    const float size = fmaxf(fmaxf(expf(scales[b]), expf(scales[b + 1])), expf(scales[b + 2]));
    const float opacity = gs_mask_sigmoid(opacities[n]);
    // (a NaN anywhere compares false, as in torch: the gaussian is frozen)
    const bool keep = moved > motion_min && size > scale_min && size < scale_max && opacity > opacity_min;
    const float k = keep ? 1.f : 0.f;  // mask.float() * omega: a non-finite omega under a zero mask stays non-finite
    float4 o = load_row4<VEC4>(omega, n);
    o.x *= k; o.y *= k; o.z *= k; o.w *= k;
    mask[n] = keep ? 1 : 0;
    store_row4<VEC4>(omega_new, n, o);
}

template <bool VEC4>
__global__ void __launch_bounds__(GS_BLOCK) stg_freeze_grads_kernel(uint32_t N, const uint8_t *__restrict__ mask,
                                                                    float *__restrict__ omega_grad, float *__restrict__ quats_grad) {
    const uint32_t n = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (n >= N) return;
    const bool keep = mask[n] != 0;
    const float ko = keep ? 1.f : 0.f, kq = keep ? 0.f : 1.f;  // multiplied, not selected: NaN * 0 = NaN as in grad * mask
    float4 o = load_row4<VEC4>(omega_grad, n), q = load_row4<VEC4>(quats_grad, n);
    o.x *= ko; o.y *= ko; o.z *= ko; o.w *= ko;
    q.x *= kq; q.y *= kq; q.z *= kq; q.w *= kq;
    store_row4<VEC4>(omega_grad, n, o);
    store_row4<VEC4>(quats_grad, n, q);
}

}  // namespace

extern "C" int32_t gs_relocation(uint32_t N, const float *opacities, const float *scales, const int32_t *ratios, const float *binoms,
                                 uint32_t n_max, float *new_opacities, float *new_scales, gs_stream_t stream) {
    GS_CHECK_ARG(n_max >= 1, "n_max must be at least 1 (binoms is [n_max, n_max])");
    if (N == 0) return 0;
    GS_CHECK_ARG(opacities && scales && ratios && binoms && new_opacities && new_scales, "null pointer");
    hipLaunchKernelGGL(relocation_kernel, dim3(gs_div_up(N, GS_BLOCK)), dim3(GS_BLOCK), 0, (hipStream_t)stream, N, opacities, scales,
                       ratios, binoms, n_max, new_opacities, new_scales);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_inject_noise(uint32_t N, float *means, const float *quats, const float *scales, const float *opacities,
                                   const float *noise, float scaler, gs_stream_t stream) {
    if (N == 0) return 0;
    GS_CHECK_ARG(means && quats && scales && opacities && noise, "null pointer");
    GS_CHECK_ARG(((uintptr_t)means | (uintptr_t)quats | (uintptr_t)scales | (uintptr_t)opacities | (uintptr_t)noise) % 4 == 0,
                 "float arrays must be 4-byte aligned");
    const dim3 grid(gs_div_up(N, GS_BLOCK)), block(GS_BLOCK);
    if ((uintptr_t)quats % 16 == 0)
        hipLaunchKernelGGL(inject_noise_kernel<true>, grid, block, 0, (hipStream_t)stream, N, means, quats, scales, opacities, noise, scaler);
    else
        hipLaunchKernelGGL(inject_noise_kernel<false>, grid, block, 0, (hipStream_t)stream, N, means, quats, scales, opacities, noise, scaler);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_densify_stats(uint32_t C, uint32_t N, uint64_t nnz, const float *grad, uint64_t grad_row_stride,
                                    const int32_t *radii, const int64_t *gaussian_ids, float sx, float sy, float extent, float *grad2d,
                                    float *count, float *radii_state, gs_stream_t stream) {
    GS_CHECK_ARG(C >= 1, "C must be at least 1");
    GS_CHECK_ARG(grad_row_stride >= 2, "grad_row_stride must be at least 2 floats");
    GS_CHECK_ARG(radii_state == nullptr || extent > 0.f, "extent (max(width, height)) must be positive");
    const bool packed = gaussian_ids != nullptr;
    if (N == 0 || (packed && nnz == 0)) return 0;
    GS_CHECK_ARG(grad && radii, "null grad / radii");
    GS_CHECK_ARG(grad2d && count, "null grad2d / count");
    GS_CHECK_ARG(((uintptr_t)grad | (uintptr_t)grad2d | (uintptr_t)count | (uintptr_t)radii_state | (uintptr_t)radii) % 4 == 0,
                 "arrays must be 4-byte aligned");
    GS_CHECK_ARG(!packed || (uintptr_t)gaussian_ids % 8 == 0, "gaussian_ids must be 8-byte aligned");
    const uint64_t rows = packed ? nnz : (uint64_t)C * N;
    GS_CHECK_ARG(rows <= 0xffffffffull * GS_BLOCK, "too many rows");
    const bool vec2 = (uintptr_t)grad % 8 == 0 && grad_row_stride % 2 == 0;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 block(GS_BLOCK);
    if (packed) {
        const dim3 grid(gs_div_up(nnz, GS_BLOCK));
        if (vec2)
            hipLaunchKernelGGL(densify_stats_packed_kernel<true>, grid, block, 0, st, nnz, N, grad, grad_row_stride, radii, gaussian_ids,
                               sx, sy, extent, grad2d, count, radii_state);
        else
            hipLaunchKernelGGL(densify_stats_packed_kernel<false>, grid, block, 0, st, nnz, N, grad, grad_row_stride, radii, gaussian_ids,
                               sx, sy, extent, grad2d, count, radii_state);
    } else {
        const dim3 grid(gs_div_up(N, GS_BLOCK));
        if (vec2)
            hipLaunchKernelGGL(densify_stats_kernel<true>, grid, block, 0, st, C, N, grad, grad_row_stride, radii, sx, sy, extent, grad2d,
                               count, radii_state);
        else
            hipLaunchKernelGGL(densify_stats_kernel<false>, grid, block, 0, st, C, N, grad, grad_row_stride, radii, sx, sy, extent, grad2d,
                               count, radii_state);
    }
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_stg_omega_mask(uint32_t N, const float *motion, uint64_t motion_row_stride, const float *scales,
                                     const float *opacities, const float *omega, float motion_min, float scale_min, float scale_max,
                                     float opacity_min, uint8_t *mask, float *omega_new, gs_stream_t stream) {
    GS_CHECK_ARG(motion_row_stride >= 3, "motion_row_stride must be at least 3 floats");
    if (N == 0) return 0;
    GS_CHECK_ARG(motion && scales && opacities && omega, "null input");
    GS_CHECK_ARG(mask && omega_new, "null mask / omega_new");
    GS_CHECK_ARG(((uintptr_t)motion | (uintptr_t)scales | (uintptr_t)opacities | (uintptr_t)omega | (uintptr_t)omega_new) % 4 == 0,
                 "float arrays must be 4-byte aligned");
    const dim3 grid(gs_div_up(N, GS_BLOCK)), block(GS_BLOCK);
    const hipStream_t st = (hipStream_t)stream;
    if (((uintptr_t)omega | (uintptr_t)omega_new) % 16 == 0)
        hipLaunchKernelGGL(stg_omega_mask_kernel<true>, grid, block, 0, st, N, motion, motion_row_stride, scales, opacities, omega,
                           motion_min, scale_min, scale_max, opacity_min, mask, omega_new);
    else
        hipLaunchKernelGGL(stg_omega_mask_kernel<false>, grid, block, 0, st, N, motion, motion_row_stride, scales, opacities, omega,
                           motion_min, scale_min, scale_max, opacity_min, mask, omega_new);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_stg_freeze_grads(uint32_t N, const uint8_t *mask, float *omega_grad, float *quats_grad, gs_stream_t stream) {
    if (N == 0) return 0;
    GS_CHECK_ARG(mask, "null mask");
    GS_CHECK_ARG(omega_grad && quats_grad, "null omega_grad / quats_grad");
    GS_CHECK_ARG(omega_grad != quats_grad, "omega_grad and quats_grad must be different arrays");
    GS_CHECK_ARG(((uintptr_t)omega_grad | (uintptr_t)quats_grad) % 4 == 0, "float arrays must be 4-byte aligned");
    const dim3 grid(gs_div_up(N, GS_BLOCK)), block(GS_BLOCK);
    const hipStream_t st = (hipStream_t)stream;
    if (((uintptr_t)omega_grad | (uintptr_t)quats_grad) % 16 == 0)
        hipLaunchKernelGGL(stg_freeze_grads_kernel<true>, grid, block, 0, st, N, mask, omega_grad, quats_grad);
    else
        hipLaunchKernelGGL(stg_freeze_grads_kernel<false>, grid, block, 0, st, N, mask, omega_grad, quats_grad);
    GS_CHECK_LAUNCH();
    return 0;
}
