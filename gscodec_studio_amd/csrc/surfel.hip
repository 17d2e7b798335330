// surfel.hip -- 2D Gaussian splatting (surfels): projection, per-tile compositing and depth-to-normal, forward and backward
// (gs_projection_2dgs_*, gs_rasterize_2dgs_*, gs_depth_to_normal_*; semantics in include/gsplat_hip.h).
//
// Projection: one thread per (camera, splat), blockIdx.y = camera so that a wave never straddles two cameras (the pose gradient is
// summed per wave).  Compositing: one 256-lane workgroup per 16x16 tile, lane t owns pixel (t % 16, t / 16) of the tile; the tile's
// list is staged through LDS in batches of 256 splat records (every lane then reads the same record: a broadcast, no bank
// conflicts; the staging writes have odd strides).  The backward walks the list back to front from the tile's last contributing
// entry, recomputes each lane's alpha, divides the transmittance back out, reduces every gradient value over the wave with the DPP
// chains of dpp_reduce.h (totals in lane 63) and issues one atomicAdd per wave and value, only from waves that have a contributing
// lane.  This is the simple first shape: correct on every case, not yet tuned.
#include "gs_common.h"
#include "dpp_reduce.h"
#include "proj_models.h"

#define SF_BATCH 256

// ---------------------------------------------------------------------------
// projection
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(GS_BLOCK) surfel_projection_fwd_kernel(
    uint32_t N, const float *__restrict__ means, const float *__restrict__ quats, const float *__restrict__ scales,
    const float *__restrict__ viewmats, const float *__restrict__ Ks, int32_t width, int32_t height, float near_plane, float far_plane,
    float radius_clip, int32_t *__restrict__ radii, float *__restrict__ means2d, float *__restrict__ depths,
    float *__restrict__ ray_transforms, float *__restrict__ normals) {
    const uint32_t n = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (n >= N) return;
    const uint32_t c = blockIdx.y;
    const uint64_t idx = (uint64_t)c * N + n;
    const Camera cam = load_camera(viewmats, Ks, c);
    const float mx = means[n * 3], my = means[n * 3 + 1], mz = means[n * 3 + 2];
    const float ct[3] = {cam.tx, cam.ty, cam.tz};
    float p[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = cam.W.m[i][0] * mx + cam.W.m[i][1] * my + cam.W.m[i][2] * mz + ct[i];

    int32_t radius = 0;
    float M[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, m2[2] = {0.f, 0.f}, nrm[3] = {0.f, 0.f, 0.f}, depth = 0.f;
    if (!(p[2] < near_plane || p[2] > far_plane)) {
        const Mat3 Rq = quat_to_rotmat(quats[n * 4], quats[n * 4 + 1], quats[n * 4 + 2], quats[n * 4 + 3]);
        const Mat3 RR = mat3_mul(cam.W, Rq);
        const float sx = scales[n * 3], sy = scales[n * 3 + 1];
        // WH = [a | b | p], rows of M = K WH
        float WH[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            WH[i][0] = RR.m[i][0] * sx;
            WH[i][1] = RR.m[i][1] * sy;
            WH[i][2] = p[i];
        }
        float Mt[9];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Mt[j] = cam.fx * WH[0][j] + cam.cx * WH[2][j];
            Mt[3 + j] = cam.fy * WH[1][j] + cam.cy * WH[2][j];
            Mt[6 + j] = WH[2][j];
        }
        const float d = Mt[6] * Mt[6] + Mt[7] * Mt[7] - Mt[8] * Mt[8];
        if (d != 0.f) {
            const float f = 1.f / d;
            const float cx2 = f * (Mt[0] * Mt[6] + Mt[1] * Mt[7] - Mt[2] * Mt[8]);
            const float cy2 = f * (Mt[3] * Mt[6] + Mt[4] * Mt[7] - Mt[5] * Mt[8]);
            const float hx = cx2 * cx2 - f * (Mt[0] * Mt[0] + Mt[1] * Mt[1] - Mt[2] * Mt[2]);
            const float hy = cy2 * cy2 - f * (Mt[3] * Mt[3] + Mt[4] * Mt[4] - Mt[5] * Mt[5]);
            const float r = ceilf(3.f * sqrtf(fmaxf(1e-4f, fmaxf(hx, hy))));
            const bool outside = cx2 + r <= 0.f || cx2 - r >= (float)width || cy2 + r <= 0.f || cy2 - r >= (float)height;
            if (r > radius_clip && !outside) {
                radius = (int32_t)r;
                m2[0] = cx2; m2[1] = cy2;
                depth = p[2];
#pragma unroll
                for (int k = 0; k < 9; ++k) M[k] = Mt[k];
                const float facing = -(RR.m[0][2] * p[0] + RR.m[1][2] * p[1] + RR.m[2][2] * p[2]);
                const float sgn = facing > 0.f ? 1.f : -1.f;
#pragma unroll
                for (int i = 0; i < 3; ++i) nrm[i] = sgn * RR.m[i][2];
            }
        }
    }
    radii[idx] = radius;
    means2d[idx * 2] = m2[0];
    means2d[idx * 2 + 1] = m2[1];
    depths[idx] = depth;
#pragma unroll
    for (int k = 0; k < 9; ++k) ray_transforms[idx * 9 + k] = M[k];
#pragma unroll
    for (int i = 0; i < 3; ++i) normals[idx * 3 + i] = nrm[i];
}

__global__ void __launch_bounds__(GS_BLOCK) surfel_projection_bwd_kernel(
    uint32_t N, const float *__restrict__ means, const float *__restrict__ quats, const float *__restrict__ scales,
    const float *__restrict__ viewmats, const float *__restrict__ Ks, const int32_t *__restrict__ radii,
    const float *__restrict__ ray_transforms, const float *__restrict__ v_means2d, const float *__restrict__ v_depths,
    const float *__restrict__ v_normals, const float *__restrict__ v_ray_transforms, float *__restrict__ v_means,
    float *__restrict__ v_quats, float *__restrict__ v_scales, float *__restrict__ v_viewmats) {
    // (no early return: the wave reductions below need every lane)
    const uint32_t n = blockIdx.x * GS_BLOCK + threadIdx.x;
    const uint32_t c = blockIdx.y;
    const uint64_t idx = (uint64_t)c * N + (n < N ? n : 0);
    const bool live = n < N && radii[idx] > 0;
    float vR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, vt[3] = {0.f, 0.f, 0.f};
    if (live) {
        const Camera cam = load_camera(viewmats, Ks, c);
        const float *M = ray_transforms + idx * 9;
        float vM[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) vM[k] = v_ray_transforms ? v_ray_transforms[idx * 9 + k] : 0.f;
        if (v_means2d) {
            // mean2d_x = (M_u . g M_w) / d, mean2d_y = (M_v . g M_w) / d with g = diag(1, 1, -1), d = M_w . g M_w
            const float gx = v_means2d[idx * 2], gy = v_means2d[idx * 2 + 1];
            const float d = M[6] * M[6] + M[7] * M[7] - M[8] * M[8];
            const float f = 1.f / d;
            const float cx2 = f * (M[0] * M[6] + M[1] * M[7] - M[2] * M[8]);
            const float cy2 = f * (M[3] * M[6] + M[4] * M[7] - M[5] * M[8]);
            const float sg[3] = {1.f, 1.f, -1.f};
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                vM[j] += gx * f * sg[j] * M[6 + j];
                vM[3 + j] += gy * f * sg[j] * M[6 + j];
                vM[6 + j] += f * sg[j] * (gx * (M[j] - 2.f * cx2 * M[6 + j]) + gy * (M[3 + j] - 2.f * cy2 * M[6 + j]));
            }
        }
        // WH = K^T-pulled gradient: rows of M are fx WH_0 + cx WH_2, fy WH_1 + cy WH_2, WH_2
        float vWH[3][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            vWH[0][j] = cam.fx * vM[j];
            vWH[1][j] = cam.fy * vM[3 + j];
            vWH[2][j] = cam.cx * vM[j] + cam.cy * vM[3 + j] + vM[6 + j];
        }
        if (v_depths) vWH[2][2] += v_depths[idx];
        const float qw = quats[n * 4], qx = quats[n * 4 + 1], qy = quats[n * 4 + 2], qz = quats[n * 4 + 3];
        const Mat3 Rq = quat_to_rotmat(qw, qx, qy, qz);
        const float sx = scales[n * 3], sy = scales[n * 3 + 1];
        const float mx = means[n * 3], my = means[n * 3 + 1], mz = means[n * 3 + 2];
        const float mw[3] = {mx, my, mz};
        // the normal: sgn * R_c * (third column of Rq); sgn from the forward's facing test
        float vn[3] = {0.f, 0.f, 0.f};
        if (v_normals) {
            const float ct[3] = {cam.tx, cam.ty, cam.tz};
            float p[3], w3[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                p[i] = cam.W.m[i][0] * mx + cam.W.m[i][1] * my + cam.W.m[i][2] * mz + ct[i];
                w3[i] = cam.W.m[i][0] * Rq.m[0][2] + cam.W.m[i][1] * Rq.m[1][2] + cam.W.m[i][2] * Rq.m[2][2];
            }
            const float facing = -(w3[0] * p[0] + w3[1] * p[1] + w3[2] * p[2]);
            const float sgn = facing > 0.f ? 1.f : -1.f;
#pragma unroll
            for (int i = 0; i < 3; ++i) vn[i] = sgn * v_normals[idx * 3 + i];
        }
        // camera-space gradients of the three columns a = R_c u s_x, b = R_c v s_y, p = R_c mean + t, and of R_c w
        // G (camera space, columns): [va, vb, vn] -> world: R_c^T G
        Mat3 V;  // d L / d Rq
        float vmean[3], vsx = 0.f, vsy = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float ga = cam.W.m[0][i] * vWH[0][0] + cam.W.m[1][i] * vWH[1][0] + cam.W.m[2][i] * vWH[2][0];
            const float gb = cam.W.m[0][i] * vWH[0][1] + cam.W.m[1][i] * vWH[1][1] + cam.W.m[2][i] * vWH[2][1];
            const float gp = cam.W.m[0][i] * vWH[0][2] + cam.W.m[1][i] * vWH[1][2] + cam.W.m[2][i] * vWH[2][2];
            const float gn = cam.W.m[0][i] * vn[0] + cam.W.m[1][i] * vn[1] + cam.W.m[2][i] * vn[2];
            V.m[i][0] = ga * sx;
            V.m[i][1] = gb * sy;
            V.m[i][2] = gn;
            vsx += ga * Rq.m[i][0];
            vsy += gb * Rq.m[i][1];
            vmean[i] = gp;
        }
        float vq[4] = {0.f, 0.f, 0.f, 0.f};
        rotmat_vjp_quat(qw, qx, qy, qz, V, vq);
#pragma unroll
        for (int i = 0; i < 3; ++i) atomicAdd(v_means + n * 3 + i, vmean[i]);
#pragma unroll
        for (int i = 0; i < 4; ++i) atomicAdd(v_quats + n * 4 + i, vq[i]);
        atomicAdd(v_scales + n * 3, vsx);
        atomicAdd(v_scales + n * 3 + 1, vsy);
        if (v_viewmats) {
            // R_c enters a, b, p and the normal: v_Rc = va (s_x u)^T + vb (s_y v)^T + vp mean^T + vn w^T ; v_t = vp
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    vR[i * 3 + j] = vWH[i][0] * sx * Rq.m[j][0] + vWH[i][1] * sy * Rq.m[j][1] + vWH[i][2] * mw[j] + vn[i] * Rq.m[j][2];
                vt[i] = vWH[i][2];
            }
        }
    }
    if (v_viewmats && __any(live)) {
        wave_reduce_sum_9(vR[0], vR[1], vR[2], vR[3], vR[4], vR[5], vR[6], vR[7], vR[8]);
        wave_reduce_sum_3(vt[0], vt[1], vt[2]);
        if ((threadIdx.x & 63) == 63) {
            float *o = v_viewmats + c * 16;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) atomicAdd(o + i * 4 + j, vR[i * 3 + j]);
                atomicAdd(o + i * 4 + 3, vt[i]);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// compositing
// ---------------------------------------------------------------------------
struct SurfelTile {
    uint32_t cam, tile, px_i, px_j;
    bool inside;
    int32_t begin, end;
    uint64_t pix;  // flat pixel index cam * H * W + i * W + j (clamped to a valid pixel for lanes outside the image)
};

GS_DEV SurfelTile surfel_tile(uint32_t C, uint32_t width, uint32_t height, uint32_t tile_width, uint32_t tile_height, uint32_t n_isects,
                              const int32_t *tile_offsets) {
    SurfelTile t;
    t.cam = blockIdx.z;
    t.tile = blockIdx.y * tile_width + blockIdx.x;
    t.px_i = blockIdx.y * 16 + (threadIdx.x >> 4);
    t.px_j = blockIdx.x * 16 + (threadIdx.x & 15);
    t.inside = t.px_i < height && t.px_j < width;
    const uint32_t n_tiles = tile_width * tile_height;
    const uint64_t slot = (uint64_t)t.cam * n_tiles + t.tile;
    t.begin = tile_offsets[slot];
    t.end = (t.cam == C - 1 && t.tile == n_tiles - 1) ? (int32_t)n_isects : tile_offsets[slot + 1];
    const uint32_t ci = t.px_i < height ? t.px_i : height - 1, cj = t.px_j < width ? t.px_j : width - 1;
    t.pix = ((uint64_t)t.cam * height + ci) * width + cj;
    return t;
}

// alpha of one splat record at one pixel; false: the splat does not contribute (zeta_z == 0 or alpha < 1/255)
struct SurfelEval {
    float hu[3], hv[3], zeta_z, s[2], dx, dy, G, alpha, raw;
    bool use3d;
};

GS_DEV bool surfel_eval(const float *M, float mx, float my, float opac, float px, float py, SurfelEval &e) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e.hu[k] = px * M[6 + k] - M[k];
        e.hv[k] = py * M[6 + k] - M[3 + k];
    }
    const float zx = e.hu[1] * e.hv[2] - e.hu[2] * e.hv[1];
    const float zy = e.hu[2] * e.hv[0] - e.hu[0] * e.hv[2];
    e.zeta_z = e.hu[0] * e.hv[1] - e.hu[1] * e.hv[0];
    if (e.zeta_z == 0.f) return false;
    e.s[0] = zx / e.zeta_z;
    e.s[1] = zy / e.zeta_z;
    const float w3 = e.s[0] * e.s[0] + e.s[1] * e.s[1];
    e.dx = mx - px;
    e.dy = my - py;
    const float w2 = 2.f * (e.dx * e.dx + e.dy * e.dy);
    e.use3d = w3 <= w2;
    const float sigma = 0.5f * (e.use3d ? w3 : w2);
    e.G = __expf(-sigma);
    e.raw = opac * e.G;
    e.alpha = fminf(GS_ALPHA_MAX, e.raw);
    return !(sigma < 0.f || e.alpha < GS_ALPHA_MIN);
}

template <int CH>
__global__ void __launch_bounds__(SF_BATCH) surfel_rasterize_fwd_kernel(
    uint32_t C, uint32_t n_isects, const float *__restrict__ means2d, const float *__restrict__ ray_transforms,
    const float *__restrict__ colors, const float *__restrict__ opacities, const float *__restrict__ normals,
    const float *__restrict__ backgrounds, const uint8_t *__restrict__ masks, uint32_t width, uint32_t height, uint32_t tile_width,
    uint32_t tile_height, const int32_t *__restrict__ tile_offsets, const int32_t *__restrict__ flatten_ids, int32_t distloss,
    float *__restrict__ render_colors, float *__restrict__ render_alphas, float *__restrict__ render_normals,
    float *__restrict__ render_distort, float *__restrict__ render_median, int32_t *__restrict__ last_ids,
    int32_t *__restrict__ median_ids) {
    __shared__ float s_geo[SF_BATCH * 12];  // mean2d (2), opacity, M (9)
    __shared__ float s_att[SF_BATCH * (CH + 3)];  // colours, normal
    const SurfelTile t = surfel_tile(C, width, height, tile_width, tile_height, n_isects, tile_offsets);
    const uint32_t tr = threadIdx.x;
    const float px = (float)t.px_j + 0.5f, py = (float)t.px_i + 0.5f;
    const bool masked = masks != nullptr && masks[(uint64_t)t.cam * tile_width * tile_height + t.tile] == 0;
    const int32_t end = masked ? t.begin : t.end;

    bool done = !t.inside;
    float T = 1.f, pix[CH], nrm[3] = {0.f, 0.f, 0.f}, distort = 0.f, acc_wd = 0.f, median = 0.f;
    int32_t last = -1, median_id = -1;
#pragma unroll
    for (int k = 0; k < CH; ++k) pix[k] = 0.f;

    for (int32_t base = t.begin; base < end; base += SF_BATCH) {
        if (__syncthreads_count(done) >= SF_BATCH) break;
        const int32_t idx = base + (int32_t)tr;
        if (idx < end) {
            const uint32_t g = (uint32_t)flatten_ids[idx];
            float *geo = s_geo + tr * 12;
            geo[0] = means2d[(uint64_t)g * 2];
            geo[1] = means2d[(uint64_t)g * 2 + 1];
            geo[2] = opacities[g];
#pragma unroll
            for (int k = 0; k < 9; ++k) geo[3 + k] = ray_transforms[(uint64_t)g * 9 + k];
            float *att = s_att + tr * (CH + 3);
#pragma unroll
            for (int k = 0; k < CH; ++k) att[k] = colors[(uint64_t)g * CH + k];
#pragma unroll
            for (int k = 0; k < 3; ++k) att[CH + k] = normals[(uint64_t)g * 3 + k];
        }
        __syncthreads();
        const int32_t count = min((int32_t)SF_BATCH, end - base);
        for (int32_t j = 0; j < count && !done; ++j) {
            const float *geo = s_geo + j * 12;
            SurfelEval e;
            if (!surfel_eval(geo + 3, geo[0], geo[1], geo[2], px, py, e)) continue;
            const float next_T = T * (1.f - e.alpha);
            if (next_T <= GS_T_MIN) {
                done = true;
                break;
            }
            const float w = e.alpha * T;
            const float *att = s_att + j * (CH + 3);
#pragma unroll
            for (int k = 0; k < CH; ++k) pix[k] += att[k] * w;
#pragma unroll
            for (int k = 0; k < 3; ++k) nrm[k] += att[CH + k] * w;
            const float depth = att[CH - 1];
            if (distloss) {
                distort += 2.f * (w * depth * (1.f - T) - w * acc_wd);
                acc_wd += w * depth;
            }
            if (T > 0.5f) {
                median = depth;
                median_id = base + j;
            }
            last = base + j;
            T = next_T;
        }
    }
    if (t.inside) {
        render_alphas[t.pix] = 1.f - T;
#pragma unroll
        for (int k = 0; k < CH; ++k)
            render_colors[t.pix * CH + k] = backgrounds ? pix[k] + T * backgrounds[t.cam * CH + k] : pix[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) render_normals[t.pix * 3 + k] = nrm[k];
        render_distort[t.pix] = distort;
        render_median[t.pix] = median;
        last_ids[t.pix] = last;
        median_ids[t.pix] = median_id;
    }
}

template <int CH>
__global__ void __launch_bounds__(SF_BATCH) surfel_rasterize_bwd_kernel(
    uint32_t C, uint32_t n_isects, const float *__restrict__ means2d, const float *__restrict__ ray_transforms,
    const float *__restrict__ colors, const float *__restrict__ opacities, const float *__restrict__ normals,
    const float *__restrict__ backgrounds, const uint8_t *__restrict__ masks, uint32_t width, uint32_t height, uint32_t tile_width,
    uint32_t tile_height, const int32_t *__restrict__ tile_offsets, const int32_t *__restrict__ flatten_ids, int32_t distloss,
    const float *__restrict__ render_colors, const float *__restrict__ render_alphas, const int32_t *__restrict__ last_ids,
    const int32_t *__restrict__ median_ids, const float *__restrict__ v_render_colors, const float *__restrict__ v_render_alphas,
    const float *__restrict__ v_render_normals, const float *__restrict__ v_render_distort, const float *__restrict__ v_render_median,
    float *__restrict__ v_means2d, float *__restrict__ v_means2d_abs, float *__restrict__ v_ray_transforms, float *__restrict__ v_colors,
    float *__restrict__ v_opacities, float *__restrict__ v_normals) {
    __shared__ float s_geo[SF_BATCH * 12];
    __shared__ float s_att[SF_BATCH * (CH + 3)];
    __shared__ int32_t s_id[SF_BATCH];
    __shared__ int32_t s_last[SF_BATCH / GS_WAVE];
    const SurfelTile t = surfel_tile(C, width, height, tile_width, tile_height, n_isects, tile_offsets);
    const uint32_t tr = threadIdx.x;
    const float px = (float)t.px_j + 0.5f, py = (float)t.px_i + 0.5f;
    const bool masked = masks != nullptr && masks[(uint64_t)t.cam * tile_width * tile_height + t.tile] == 0;

    // (lanes outside the image read a valid pixel's values and never use them: my_last = -1 keeps them out)
    const int32_t my_last = (t.inside && !masked) ? last_ids[t.pix] : -1;
    const int32_t my_median = t.inside ? median_ids[t.pix] : -1;
    const float T_final = 1.f - render_alphas[t.pix];
    float T = T_final;
    float v_c[CH], v_n[3], bg_dot = 0.f;
#pragma unroll
    for (int k = 0; k < CH; ++k) v_c[k] = v_render_colors ? v_render_colors[t.pix * CH + k] : 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) v_n[k] = v_render_normals ? v_render_normals[t.pix * 3 + k] : 0.f;
    const float v_a = v_render_alphas ? v_render_alphas[t.pix] : 0.f;
    const float v_med = v_render_median ? v_render_median[t.pix] : 0.f;
    const bool dist = distloss && v_render_distort != nullptr;
    const float v_dist = dist ? v_render_distort[t.pix] : 0.f;
    if (backgrounds) {
#pragma unroll
        for (int k = 0; k < CH; ++k) bg_dot += backgrounds[t.cam * CH + k] * v_c[k];
    }
    // what the splats behind the current one contributed: sum w x (colours, normals), sum w, sum w d, sum g w (distortion)
    float beh_c[CH], beh_n[3] = {0.f, 0.f, 0.f}, beh_w = 0.f, beh_wd = 0.f, beh_gw = 0.f;
#pragma unroll
    for (int k = 0; k < CH; ++k) beh_c[k] = 0.f;
    // total sum w d of the pixel: the accumulated last channel without its background share
    float tot_wd = 0.f;
    if (dist) tot_wd = render_colors[t.pix * CH + CH - 1] - (backgrounds ? T_final * backgrounds[t.cam * CH + CH - 1] : 0.f);

    const int32_t wave_last = wave_max_i32(my_last);
    if ((tr & 63) == 63) s_last[tr >> 6] = wave_last;
    __syncthreads();
    int32_t tile_last = s_last[0];
#pragma unroll
    for (int k = 1; k < SF_BATCH / GS_WAVE; ++k) tile_last = max(tile_last, s_last[k]);

    // batches from the tile's last contributing entry down to the head of its list; slot j of a batch holds entry top - j
    for (int32_t top = tile_last; top >= t.begin; top -= SF_BATCH) {
        __syncthreads();
        const int32_t idx = top - (int32_t)tr;
        if (idx >= t.begin) {
            const uint32_t g = (uint32_t)flatten_ids[idx];
            s_id[tr] = (int32_t)g;
            float *geo = s_geo + tr * 12;
            geo[0] = means2d[(uint64_t)g * 2];
            geo[1] = means2d[(uint64_t)g * 2 + 1];
            geo[2] = opacities[g];
#pragma unroll
            for (int k = 0; k < 9; ++k) geo[3 + k] = ray_transforms[(uint64_t)g * 9 + k];
            float *att = s_att + tr * (CH + 3);
#pragma unroll
            for (int k = 0; k < CH; ++k) att[k] = colors[(uint64_t)g * CH + k];
#pragma unroll
            for (int k = 0; k < 3; ++k) att[CH + k] = normals[(uint64_t)g * 3 + k];
        }
        __syncthreads();
        const int32_t count = min((int32_t)SF_BATCH, top - t.begin + 1);
        for (int32_t j = max(0, top - wave_last); j < count; ++j) {  // (wave-uniform bounds)
            const int32_t entry = top - j;
            const float *geo = s_geo + j * 12;
            const float *att = s_att + j * (CH + 3);
            SurfelEval e;
            bool valid = entry <= my_last;
            if (valid) valid = surfel_eval(geo + 3, geo[0], geo[1], geo[2], px, py, e);
            if (!__any(valid)) continue;

            float g_c[4] = {0.f, 0.f, 0.f, 0.f}, g_n[3] = {0.f, 0.f, 0.f}, g_M[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            float g_xy[2] = {0.f, 0.f}, g_abs[2] = {0.f, 0.f}, g_o = 0.f;
            if (valid) {
                const float ra = 1.f / (1.f - e.alpha);
                T *= ra;  // transmittance in front of this splat
                const float w = e.alpha * T;
                const float depth = att[CH - 1];
                float v_alpha = 0.f;
#pragma unroll
                for (int k = 0; k < CH; ++k) {
                    g_c[k] = w * v_c[k];
                    v_alpha += (att[k] * T - beh_c[k] * ra) * v_c[k];
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    g_n[k] = w * v_n[k];
                    v_alpha += (att[CH + k] * T - beh_n[k] * ra) * v_n[k];
                }
                v_alpha += T_final * ra * (v_a - bg_dot);
                if (entry == my_median) g_c[CH - 1] += v_med;
                if (dist) {
                    // L = 2 sum_i sum_{j<i} w_i w_j (d_i - d_j):  d L / d w_k = 2 (d_k A_k - D_k + D_behind - d_k A_behind) with
                    // A_k = 1 - T_k, D_k = sum_{j<k} w_j d_j = D_total - D_behind - w_k d_k;  d L / d d_k = 2 w_k (A_k - A_behind)
                    const float A_k = 1.f - T;
                    const float D_k = tot_wd - beh_wd - w * depth;
                    const float g_w = 2.f * (depth * A_k - D_k + beh_wd - depth * beh_w);
                    v_alpha += (g_w * T - beh_gw * ra) * v_dist;
                    g_c[CH - 1] += 2.f * w * (A_k - beh_w) * v_dist;
                    beh_gw += g_w * w;
                    beh_wd += w * depth;
                }
                beh_w += w;
                if (e.raw <= GS_ALPHA_MAX) {
                    g_o = e.G * v_alpha;
                    const float v_G = geo[2] * v_alpha;
                    if (e.use3d) {
                        // G = exp(-(s.s) / 2), s = zeta_xy / zeta_z, zeta = h_u x h_v
                        const float vsx = -e.G * v_G * e.s[0] / e.zeta_z, vsy = -e.G * v_G * e.s[1] / e.zeta_z;
                        const float vz[3] = {vsx, vsy, -(vsx * e.s[0] + vsy * e.s[1])};
                        // v_hu = h_v x v_zeta ; v_hv = v_zeta x h_u
                        const float vhu[3] = {e.hv[1] * vz[2] - e.hv[2] * vz[1], e.hv[2] * vz[0] - e.hv[0] * vz[2],
                                              e.hv[0] * vz[1] - e.hv[1] * vz[0]};
                        const float vhv[3] = {vz[1] * e.hu[2] - vz[2] * e.hu[1], vz[2] * e.hu[0] - vz[0] * e.hu[2],
                                              vz[0] * e.hu[1] - vz[1] * e.hu[0]};
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            g_M[k] = -vhu[k];
                            g_M[3 + k] = -vhv[k];
                            g_M[6 + k] = px * vhu[k] + py * vhv[k];
                        }
                    } else {
                        // G = exp(-|mean2d - p|^2)
                        g_xy[0] = -2.f * e.G * v_G * e.dx;
                        g_xy[1] = -2.f * e.G * v_G * e.dy;
                        g_abs[0] = fabsf(g_xy[0]);
                        g_abs[1] = fabsf(g_xy[1]);
                    }
                }
#pragma unroll
                for (int k = 0; k < CH; ++k) beh_c[k] += att[k] * w;
#pragma unroll
                for (int k = 0; k < 3; ++k) beh_n[k] += att[CH + k] * w;
            }
            wave_reduce_sum_9(g_M[0], g_M[1], g_M[2], g_M[3], g_M[4], g_M[5], g_M[6], g_M[7], g_M[8]);
            wave_reduce_sum_5(g_xy[0], g_xy[1], g_abs[0], g_abs[1], g_o);
            wave_reduce_sum_7(g_c[0], g_c[1], g_c[2], g_c[3], g_n[0], g_n[1], g_n[2]);
            if ((tr & 63) == 63) {
                const uint64_t g = (uint64_t)(uint32_t)s_id[j];
#pragma unroll
                for (int k = 0; k < 9; ++k) atomicAdd(v_ray_transforms + g * 9 + k, g_M[k]);
                atomicAdd(v_means2d + g * 2, g_xy[0]);
                atomicAdd(v_means2d + g * 2 + 1, g_xy[1]);
                if (v_means2d_abs) {
                    atomicAdd(v_means2d_abs + g * 2, g_abs[0]);
                    atomicAdd(v_means2d_abs + g * 2 + 1, g_abs[1]);
                }
                atomicAdd(v_opacities + g, g_o);
#pragma unroll
                for (int k = 0; k < CH; ++k) atomicAdd(v_colors + g * CH + k, g_c[k]);
#pragma unroll
                for (int k = 0; k < 3; ++k) atomicAdd(v_normals + g * 3 + k, g_n[k]);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// depth -> normal
// ---------------------------------------------------------------------------
// Its own struct, not Camera: the rotation here is camera->world, Camera::W is world->camera
struct DepthCam {
    Mat3 R;
    float fx, fy, cx, cy;
    int z_depth;
};

GS_DEV DepthCam depth_cam(const float *c2w, const float *K, int z_depth) {
    const Mat3 R = load_rot(c2w);
    Camera k;
    load_intrinsics(k, K);
    return {R, k.fx, k.fy, k.cx, k.cy, z_depth};
}

// world-space ray direction of pixel (i, j): the point is origin + depth * dir, and the origin cancels in the differences
GS_DEV void depth_dir(const DepthCam &c, int i, int j, float dir[3]) {
    const float x = ((float)j - c.cx + 0.5f) / c.fx, y = ((float)i - c.cy + 0.5f) / c.fy;
#pragma unroll
    for (int k = 0; k < 3; ++k) dir[k] = c.R.m[k][0] * x + c.R.m[k][1] * y + c.R.m[k][2];
    if (!c.z_depth) {
        const float inv = 1.f / fmaxf(sqrtf(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]), 1e-12f);
#pragma unroll
        for (int k = 0; k < 3; ++k) dir[k] *= inv;
    }
}

// the two central differences of interior pixel (i, j)
GS_DEV void depth_diffs(const DepthCam &c, const float *d, int W, int i, int j, float dx[3], float dy[3]) {
    float a[3], b[3];
    depth_dir(c, i + 1, j, a);
    depth_dir(c, i - 1, j, b);
    const float da = d[(i + 1) * W + j], db = d[(i - 1) * W + j];
#pragma unroll
    for (int k = 0; k < 3; ++k) dx[k] = da * a[k] - db * b[k];
    depth_dir(c, i, j + 1, a);
    depth_dir(c, i, j - 1, b);
    const float dc = d[i * W + j + 1], dd = d[i * W + j - 1];
#pragma unroll
    for (int k = 0; k < 3; ++k) dy[k] = dc * a[k] - dd * b[k];
}

__global__ void __launch_bounds__(GS_BLOCK) depth_to_normal_fwd_kernel(uint32_t H, uint32_t W, const float *__restrict__ depths,
                                                                     const float *__restrict__ camtoworlds, const float *__restrict__ Ks,
                                                                     int32_t z_depth, float *__restrict__ normals) {
    const uint32_t p = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (p >= H * W) return;
    const uint32_t b = blockIdx.y;
    const int i = (int)(p / W), j = (int)(p % W);
    float n[3] = {0.f, 0.f, 0.f};
    if (i >= 1 && j >= 1 && i + 1 < (int)H && j + 1 < (int)W) {
        const DepthCam c = depth_cam(camtoworlds + b * 16, Ks + b * 9, z_depth);
        float dx[3], dy[3];
        depth_diffs(c, depths + (uint64_t)b * H * W, (int)W, i, j, dx, dy);
        const float cr[3] = {dx[1] * dy[2] - dx[2] * dy[1], dx[2] * dy[0] - dx[0] * dy[2], dx[0] * dy[1] - dx[1] * dy[0]};
        const float inv = 1.f / fmaxf(sqrtf(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]), 1e-12f);
#pragma unroll
        for (int k = 0; k < 3; ++k) n[k] = cr[k] * inv;
    }
    float *o = normals + ((uint64_t)b * H * W + p) * 3;
    o[0] = n[0]; o[1] = n[1]; o[2] = n[2];
}

// gradients of interior pixel (i, j)'s normal with respect to its two differences
GS_DEV void depth_normal_vjp(const DepthCam &c, const float *d, const float *v_normals, int W, int i, int j, float vdx[3], float vdy[3]) {
    float dx[3], dy[3];
    depth_diffs(c, d, W, i, j, dx, dy);
    const float cr[3] = {dx[1] * dy[2] - dx[2] * dy[1], dx[2] * dy[0] - dx[0] * dy[2], dx[0] * dy[1] - dx[1] * dy[0]};
    const float len = sqrtf(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
    const float *vn = v_normals + ((uint64_t)i * W + j) * 3;
    float vc[3];
    if (len > 1e-12f) {
        const float inv = 1.f / len;
        const float n[3] = {cr[0] * inv, cr[1] * inv, cr[2] * inv};
        const float dot = n[0] * vn[0] + n[1] * vn[1] + n[2] * vn[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) vc[k] = (vn[k] - n[k] * dot) * inv;
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) vc[k] = vn[k] * 1e12f;
    }
    // c = dx x dy: v_dx = dy x v_c, v_dy = v_c x dx
    vdx[0] = dy[1] * vc[2] - dy[2] * vc[1];
    vdx[1] = dy[2] * vc[0] - dy[0] * vc[2];
    vdx[2] = dy[0] * vc[1] - dy[1] * vc[0];
    vdy[0] = vc[1] * dx[2] - vc[2] * dx[1];
    vdy[1] = vc[2] * dx[0] - vc[0] * dx[2];
    vdy[2] = vc[0] * dx[1] - vc[1] * dx[0];
}

__global__ void __launch_bounds__(GS_BLOCK) depth_to_normal_bwd_kernel(uint32_t H, uint32_t W, const float *__restrict__ depths,
                                                                     const float *__restrict__ camtoworlds, const float *__restrict__ Ks,
                                                                     int32_t z_depth, const float *__restrict__ v_normals,
                                                                     float *__restrict__ v_depths) {
    const uint32_t p = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (p >= H * W) return;
    const uint32_t b = blockIdx.y;
    const int i = (int)(p / W), j = (int)(p % W), h = (int)H, w = (int)W;
    const DepthCam c = depth_cam(camtoworlds + b * 16, Ks + b * 9, z_depth);
    const float *d = depths + (uint64_t)b * H * W;
    const float *vn = v_normals + (uint64_t)b * H * W * 3;
    // this pixel's point is the "+" end of dx for (i - 1, j), the "-" end for (i + 1, j), the "+" end of dy for (i, j - 1), the
    // "-" end for (i, j + 1) -- where those pixels are interior
    float vP[3] = {0.f, 0.f, 0.f}, a[3], bb[3];
    const bool col_in = j >= 1 && j + 1 < w, row_in = i >= 1 && i + 1 < h;
    if (col_in && i - 1 >= 1 && i < h) {  // (i - 1, j) interior: i - 1 >= 1 and i - 1 + 1 < h
        depth_normal_vjp(c, d, vn, w, i - 1, j, a, bb);
#pragma unroll
        for (int k = 0; k < 3; ++k) vP[k] += a[k];
    }
    if (col_in && i + 1 + 1 < h) {  // (i + 1, j) interior (i + 1 >= 1 always)
        depth_normal_vjp(c, d, vn, w, i + 1, j, a, bb);
#pragma unroll
        for (int k = 0; k < 3; ++k) vP[k] -= a[k];
    }
    if (row_in && j - 1 >= 1) {  // (i, j - 1) interior: j - 1 + 1 < w holds
        depth_normal_vjp(c, d, vn, w, i, j - 1, a, bb);
#pragma unroll
        for (int k = 0; k < 3; ++k) vP[k] += bb[k];
    }
    if (row_in && j + 1 + 1 < w) {  // (i, j + 1) interior
        depth_normal_vjp(c, d, vn, w, i, j + 1, a, bb);
#pragma unroll
        for (int k = 0; k < 3; ++k) vP[k] -= bb[k];
    }
    float dir[3];
    depth_dir(c, i, j, dir);
    v_depths[(uint64_t)b * H * W + p] = dir[0] * vP[0] + dir[1] * vP[1] + dir[2] * vP[2];
}

// ---------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------
extern "C" int32_t gs_projection_2dgs_fwd(uint32_t C, uint32_t N, const float *means, const float *quats, const float *scales,
                                          const float *viewmats, const float *Ks, int32_t width, int32_t height, float eps2d,
                                          float near_plane, float far_plane, float radius_clip, int32_t *radii, float *means2d,
                                          float *depths, float *ray_transforms, float *normals, gs_stream_t stream) {
    (void)eps2d;
    if (C == 0 || N == 0) return 0;
    GS_CHECK_ARG(means && quats && scales && viewmats && Ks, "null input pointer");
    GS_CHECK_ARG(radii && means2d && depths && ray_transforms && normals, "null output pointer");
    GS_CHECK_ARG(width > 0 && height > 0, "empty image");
    GS_CHECK_ARG(C <= 65535, "more than 65535 cameras");
    hipLaunchKernelGGL(surfel_projection_fwd_kernel, dim3(gs_div_up(N, GS_BLOCK), C), dim3(GS_BLOCK), 0, (hipStream_t)stream, N, means,
                       quats, scales, viewmats, Ks, width, height, near_plane, far_plane, radius_clip, radii, means2d, depths,
                       ray_transforms, normals);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_projection_2dgs_bwd(uint32_t C, uint32_t N, const float *means, const float *quats, const float *scales,
                                          const float *viewmats, const float *Ks, const int32_t *radii, const float *ray_transforms,
                                          const float *v_means2d, const float *v_depths, const float *v_normals,
                                          const float *v_ray_transforms, float *v_means, float *v_quats, float *v_scales,
                                          float *v_viewmats, gs_stream_t stream) {
    if (C == 0 || N == 0) return 0;
    GS_CHECK_ARG(means && quats && scales && viewmats && Ks && radii && ray_transforms, "null input pointer");
    GS_CHECK_ARG(v_means && v_quats && v_scales, "v_means, v_quats and v_scales go together (none may be null)");
    GS_CHECK_ARG(C <= 65535, "more than 65535 cameras");
    hipLaunchKernelGGL(surfel_projection_bwd_kernel, dim3(gs_div_up(N, GS_BLOCK), C), dim3(GS_BLOCK), 0, (hipStream_t)stream, N, means,
                       quats, scales, viewmats, Ks, radii, ray_transforms, v_means2d, v_depths, v_normals, v_ray_transforms, v_means,
                       v_quats, v_scales, v_viewmats);
    GS_CHECK_LAUNCH();
    return 0;
}

#define SF_DISPATCH(kernel, ...)                                                                                                   \
    switch (channels) {                                                                                                            \
    case 1: hipLaunchKernelGGL(kernel<1>, grid, dim3(SF_BATCH), 0, (hipStream_t)stream, __VA_ARGS__); break;                       \
    case 2: hipLaunchKernelGGL(kernel<2>, grid, dim3(SF_BATCH), 0, (hipStream_t)stream, __VA_ARGS__); break;                       \
    case 3: hipLaunchKernelGGL(kernel<3>, grid, dim3(SF_BATCH), 0, (hipStream_t)stream, __VA_ARGS__); break;                       \
    default: hipLaunchKernelGGL(kernel<4>, grid, dim3(SF_BATCH), 0, (hipStream_t)stream, __VA_ARGS__); break;                      \
    }

static int32_t surfel_check_grid(const char *fn, uint32_t C, uint32_t channels, uint32_t width, uint32_t height, uint32_t tile_size,
                                 uint32_t tile_width, uint32_t tile_height) {
    if (channels < 1 || channels > 4) {
        gs_set_error("%s: unsupported number of colour channels %u (1..4, the depth column included)", fn, channels);
        return 1;
    }
    if (tile_size != 16) {
        gs_set_error("%s: tile_size must be 16 (got %u)", fn, tile_size);
        return 1;
    }
    if (width == 0 || height == 0 || tile_width != (width + 15) / 16 || tile_height != (height + 15) / 16) {
        gs_set_error("%s: tile grid %u x %u does not cover a %u x %u image with 16-pixel tiles", fn, tile_width, tile_height, width,
                     height);
        return 1;
    }
    if (tile_height > 65535 || C > 65535) {
        gs_set_error("%s: more than 65535 tile rows or cameras", fn);
        return 1;
    }
    return 0;
}

extern "C" int32_t gs_rasterize_2dgs_fwd(uint32_t C, uint32_t N, uint32_t n_isects, uint32_t channels, const float *means2d,
                                         const float *ray_transforms, const float *colors, const float *opacities, const float *normals,
                                         const float *backgrounds, const uint8_t *masks, uint32_t width, uint32_t height,
                                         uint32_t tile_size, uint32_t tile_width, uint32_t tile_height, const int32_t *tile_offsets,
                                         const int32_t *flatten_ids, int32_t distloss, float *render_colors, float *render_alphas,
                                         float *render_normals, float *render_distort, float *render_median, int32_t *last_ids,
                                         int32_t *median_ids, gs_stream_t stream) {
    (void)N;
    if (surfel_check_grid(__func__, C, channels, width, height, tile_size, tile_width, tile_height)) return 1;
    if (C == 0) return 0;
    GS_CHECK_ARG(tile_offsets && render_colors && render_alphas && render_normals && render_distort && render_median && last_ids &&
                     median_ids,
                 "tile_offsets and the seven outputs go together (none may be null)");
    GS_CHECK_ARG(n_isects == 0 || (means2d && ray_transforms && colors && opacities && normals && flatten_ids),
                 "n_isects > 0 needs means2d, ray_transforms, colors, opacities, normals and flatten_ids");
    GS_CHECK_ARG(n_isects < 0x7fffffffu, "n_isects must be below 2^31 - 1");
    const dim3 grid(tile_width, tile_height, C);
    SF_DISPATCH(surfel_rasterize_fwd_kernel, C, n_isects, means2d, ray_transforms, colors, opacities, normals, backgrounds, masks, width,
                height, tile_width, tile_height, tile_offsets, flatten_ids, distloss, render_colors, render_alphas, render_normals,
                render_distort, render_median, last_ids, median_ids);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_rasterize_2dgs_bwd(uint32_t C, uint32_t N, uint32_t n_isects, uint32_t channels, const float *means2d,
                                         const float *ray_transforms, const float *colors, const float *opacities, const float *normals,
                                         const float *backgrounds, const uint8_t *masks, uint32_t width, uint32_t height,
                                         uint32_t tile_size, uint32_t tile_width, uint32_t tile_height, const int32_t *tile_offsets,
                                         const int32_t *flatten_ids, int32_t distloss, const float *render_colors,
                                         const float *render_alphas, const int32_t *last_ids, const int32_t *median_ids,
                                         const float *v_render_colors, const float *v_render_alphas, const float *v_render_normals,
                                         const float *v_render_distort, const float *v_render_median, float *v_means2d,
                                         float *v_means2d_abs, float *v_ray_transforms, float *v_colors, float *v_opacities,
                                         float *v_normals, gs_stream_t stream) {
    (void)N;
    if (surfel_check_grid(__func__, C, channels, width, height, tile_size, tile_width, tile_height)) return 1;
    if (C == 0 || n_isects == 0) return 0;
    GS_CHECK_ARG(means2d && ray_transforms && colors && opacities && normals && tile_offsets && flatten_ids, "null input pointer");
    GS_CHECK_ARG(render_colors && render_alphas && last_ids && median_ids, "the forward's outputs go together (none may be null)");
    GS_CHECK_ARG(v_means2d && v_ray_transforms && v_colors && v_opacities && v_normals,
                 "v_means2d, v_ray_transforms, v_colors, v_opacities and v_normals go together (none may be null)");
    GS_CHECK_ARG(n_isects < 0x7fffffffu, "n_isects must be below 2^31 - 1");
    const dim3 grid(tile_width, tile_height, C);
    SF_DISPATCH(surfel_rasterize_bwd_kernel, C, n_isects, means2d, ray_transforms, colors, opacities, normals, backgrounds, masks, width,
                height, tile_width, tile_height, tile_offsets, flatten_ids, distloss, render_colors, render_alphas, last_ids, median_ids,
                v_render_colors, v_render_alphas, v_render_normals, v_render_distort, v_render_median, v_means2d, v_means2d_abs,
                v_ray_transforms, v_colors, v_opacities, v_normals);
    GS_CHECK_LAUNCH();
    return 0;
}

static int32_t depth_check(const char *fn, uint32_t B, uint32_t H, uint32_t W) {
    if ((uint64_t)H * W >= ((uint64_t)1 << 31) || B > 65535) {
        gs_set_error("%s: a depth map must have fewer than 2^31 pixels and the batch at most 65535 entries", fn);
        return 1;
    }
    return 0;
}

extern "C" int32_t gs_depth_to_normal_fwd(uint32_t B, uint32_t H, uint32_t W, const float *depths, const float *camtoworlds,
                                          const float *Ks, int32_t z_depth, float *normals, gs_stream_t stream) {
    if (B == 0 || H == 0 || W == 0) return 0;
    GS_CHECK_ARG(depths && camtoworlds && Ks && normals, "null pointer");
    if (depth_check(__func__, B, H, W)) return 1;
    hipLaunchKernelGGL(depth_to_normal_fwd_kernel, dim3(gs_div_up((uint64_t)H * W, GS_BLOCK), B), dim3(GS_BLOCK), 0, (hipStream_t)stream,
                       H, W, depths, camtoworlds, Ks, z_depth, normals);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_depth_to_normal_bwd(uint32_t B, uint32_t H, uint32_t W, const float *depths, const float *camtoworlds,
                                          const float *Ks, int32_t z_depth, const float *v_normals, float *v_depths,
                                          gs_stream_t stream) {
    if (B == 0 || H == 0 || W == 0) return 0;
    GS_CHECK_ARG(depths && camtoworlds && Ks && v_normals && v_depths, "null pointer");
    if (depth_check(__func__, B, H, W)) return 1;
    hipLaunchKernelGGL(depth_to_normal_bwd_kernel, dim3(gs_div_up((uint64_t)H * W, GS_BLOCK), B), dim3(GS_BLOCK), 0, (hipStream_t)stream,
                       H, W, depths, camtoworlds, Ks, z_depth, v_normals, v_depths);
    GS_CHECK_LAUNCH();
    return 0;
}
