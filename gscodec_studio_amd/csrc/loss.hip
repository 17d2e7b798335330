// loss.hip -- the trainers' photometric loss: 3DGS SSIM (11-tap Gaussian window, sigma 1.5, zero padding) and L1, forward and
// backward (gs_ssim_fwd / gs_ssim_bwd).
//
// Forward, one pass over x and y: a block owns a SSIM_TH x SSIM_TW tile of outputs of one image b and walks its C channels.  Per
// channel it stages the (TH+10) x (TW+10) halo of x and y in LDS (zero outside the image), runs the horizontal 11-tap pass over
// the five products (x, y, x^2, y^2, xy; 4 outputs per thread from 14 staged values) into LDS, then the vertical pass (4 outputs
// per thread), and evaluates the SSIM map and |x - y| per element.  With train it also writes the three coefficient maps the
// backward convolves, already masked to the averaged positions:
//   dA = dS/dmu_x,  dB = dS/dE[x^2],  dC = dS/dE[xy]      (E[x^2], E[xy] independent; the -2 mu_x / -mu_y of sigma included)
// so that dx(p) = g * sum_q w(q - p) (dA(q) + 2 x(p) dB(q) + y(p) dC(q)).  The saved maps cost 12 B per element written and read
// once more (44 B / element in all against 20 B when the backward recomputes the moments) but keep the backward at two
// 3-map passes instead of two 5-map passes plus the SSIM derivative on a tile grown by the halo (the recompute form has not been
// built; the measured times of this one are in profiles/r08_loss.txt).
// Reduction: every block writes its (sum S, sum |x - y|) in double; a second one-block launch sums the partials in a fixed order.
// No atomics: the results are bit-identical from run to run.  Each element's arithmetic and every summation order depend only on
// the logical (b, c, h, w) index -- strides only change addresses -- so an NCHW tensor and the NHWC view of the same values give
// the same bits.
// Backward, one pass: per channel the three maps' halo is staged, convolved (horizontal, then vertical, 4 outputs per thread),
// combined with x(p), y(p) and the L1 term w_l1 * g_l1 * sign(x - y) / count, and written in dx's own strides.  The upstream
// gradients are read from device memory: no host synchronisation anywhere.
#include "gs_common.h"

#include <math.h>

#define SSIM_TH 16
#define SSIM_TW 64
#define SSIM_R 5                          // window radius
#define SSIM_HR (SSIM_TH + 2 * SSIM_R)    // 26 staged rows
#define SSIM_HC (SSIM_TW + 2 * SSIM_R)    // 74 staged columns
#define SSIM_PITCH 80                     // staged row pitch: 16-B rows, and the float4 reads of the last column group stay inside
#define SSIM_RED_THREADS 1024

namespace {

constexpr float kC1 = 0.01f * 0.01f;
constexpr float kC2 = 0.03f * 0.03f;

struct Window {
    float w[11];
};

struct Geo {
    const float *x, *y;
    int64_t xs[4], ys[4];  // element strides along b, c, h, w
    uint32_t B, C, H, W;
    uint32_t valid;        // average over [5, H-5) x [5, W-5) only
};

Window make_window() {
    double g[11], s = 0.0;
    for (int i = 0; i < 11; ++i) {
        g[i] = exp(-(double)((i - 5) * (i - 5)) / 4.5);
        s += g[i];
    }
    Window w;
    for (int i = 0; i < 11; ++i) w.w[i] = (float)(g[i] / s);
    return w;
}

GS_DEV bool averaged(const Geo &g, uint32_t h, uint32_t w) {
    return !g.valid || (h >= SSIM_R && h + SSIM_R < g.H && w >= SSIM_R && w + SSIM_R < g.W);
}

// the (b, c) plane's halo tile of one or two strided tensors into LDS rows of SSIM_PITCH floats, zero outside the image
GS_DEV void stage(float *dst, const float *src, const int64_t *st, uint32_t b, uint32_t c, int32_t h0, int32_t w0, uint32_t H,
                  uint32_t W) {
    const float *base = src + (int64_t)b * st[0] + (int64_t)c * st[1];
    for (uint32_t i = threadIdx.x; i < SSIM_HR * SSIM_HC; i += GS_BLOCK) {
        const uint32_t r = i / SSIM_HC, k = i - r * SSIM_HC;
        const int32_t h = h0 - SSIM_R + (int32_t)r, w = w0 - SSIM_R + (int32_t)k;
        float v = 0.f;
        if (h >= 0 && w >= 0 && (uint32_t)h < H && (uint32_t)w < W) v = base[(int64_t)h * st[2] + (int64_t)w * st[3]];
        dst[r * SSIM_PITCH + k] = v;
    }
}

// 14 staged values of one row from column 4 * grp (four 16-B LDS reads; the last two values are not used)
GS_DEV void row14(const float *row, uint32_t grp, float v[16]) {
    const float4 *p = reinterpret_cast<const float4 *>(row + 4 * grp);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 f = p[q];
        v[4 * q + 0] = f.x;
        v[4 * q + 1] = f.y;
        v[4 * q + 2] = f.z;
        v[4 * q + 3] = f.w;
    }
}

struct SsimFwdArgs {
    Geo g;
    Window win;
    uint32_t train;
    float *maps;      // [3][B][C][H][W] (train)
    double *partials; // [blocks][2]
};

__global__ void __launch_bounds__(GS_BLOCK) ssim_fwd_kernel(SsimFwdArgs a) {
    __shared__ __attribute__((aligned(16))) float s_x[SSIM_HR * SSIM_PITCH];
    __shared__ __attribute__((aligned(16))) float s_y[SSIM_HR * SSIM_PITCH];
    __shared__ __attribute__((aligned(16))) float s_h[5][SSIM_HR * SSIM_TW];
    __shared__ double2 s_red[GS_BLOCK / GS_WAVE];  // (ssim, l1)
    const Geo &g = a.g;
    const uint32_t b = blockIdx.z;
    const int32_t h0 = (int32_t)(blockIdx.y * SSIM_TH), w0 = (int32_t)(blockIdx.x * SSIM_TW);
    const uint32_t tid = threadIdx.x;
    const uint32_t col = tid % SSIM_TW, rg = tid / SSIM_TW;  // vertical pass: rows 4 rg .. 4 rg + 3 of column col
    const uint64_t plane = (uint64_t)g.H * g.W;
    double acc_s = 0.0, acc_l = 0.0;
    for (uint32_t c = 0; c < g.C; ++c) {
        stage(s_x, g.x, g.xs, b, c, h0, w0, g.H, g.W);
        stage(s_y, g.y, g.ys, b, c, h0, w0, g.H, g.W);
        __syncthreads();
        // horizontal pass: staged row r, outputs 4 grp .. 4 grp + 3
        for (uint32_t j = tid; j < SSIM_HR * (SSIM_TW / 4); j += GS_BLOCK) {
            const uint32_t r = j / (SSIM_TW / 4), grp = j % (SSIM_TW / 4);
            float xv[16], yv[16];
            row14(s_x + r * SSIM_PITCH, grp, xv);
            row14(s_y + r * SSIM_PITCH, grp, yv);
            float o[5][4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float mx = 0.f, my = 0.f, mxx = 0.f, myy = 0.f, mxy = 0.f;
#pragma unroll
                for (int t = 0; t < 11; ++t) {
                    const float wt = a.win.w[t], xx = xv[k + t], yy = yv[k + t];
                    mx += wt * xx;
                    my += wt * yy;
                    mxx += wt * (xx * xx);
                    myy += wt * (yy * yy);
                    mxy += wt * (xx * yy);
                }
                o[0][k] = mx;
                o[1][k] = my;
                o[2][k] = mxx;
                o[3][k] = myy;
                o[4][k] = mxy;
            }
#pragma unroll
            for (int m = 0; m < 5; ++m)
                *reinterpret_cast<float4 *>(&s_h[m][r * SSIM_TW + 4 * grp]) = make_float4(o[m][0], o[m][1], o[m][2], o[m][3]);
        }
        __syncthreads();
        // vertical pass: 4 outputs per thread from 14 rows of each of the five maps
        float mom[5][4];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            float v[14];
#pragma unroll
            for (int i = 0; i < 14; ++i) v[i] = s_h[m][(4 * rg + i) * SSIM_TW + col];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float s = 0.f;
#pragma unroll
                for (int t = 0; t < 11; ++t) s += a.win.w[t] * v[k + t];
                mom[m][k] = s;
            }
        }
        const uint32_t ow = (uint32_t)w0 + col;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t oh = (uint32_t)h0 + 4 * rg + k;
            if (oh >= g.H || ow >= g.W) continue;
            const float xc = s_x[(4 * rg + k + SSIM_R) * SSIM_PITCH + col + SSIM_R];
            const float yc = s_y[(4 * rg + k + SSIM_R) * SSIM_PITCH + col + SSIM_R];
            acc_l += (double)fabsf(xc - yc);
            const float mu1 = mom[0][k], mu2 = mom[1][k];
            const float mu1sq = mu1 * mu1, mu2sq = mu2 * mu2, mu12 = mu1 * mu2;
            const float s11 = mom[2][k] - mu1sq, s22 = mom[3][k] - mu2sq, s12 = mom[4][k] - mu12;
            const float A = 2.f * mu12 + kC1, Bn = 2.f * s12 + kC2;
            const float Cd = mu1sq + mu2sq + kC1, D = s11 + s22 + kC2;
            const float den = Cd * D;
            const float S = (A * Bn) / den;
            const bool avg = averaged(g, oh, ow);
            if (avg) acc_s += (double)S;
            if (a.train) {
                float dA = 0.f, dB = 0.f, dC = 0.f;
                if (avg) {
                    // S = A Bn / (Cd D): dS/dmu1 = S (2 mu2 / A - 2 mu2 / Bn - 2 mu1 / Cd + 2 mu1 / D), written without the
                    // divisions by A and Bn (both can be tiny); dS/dE[x^2] = -S / D; dS/dE[xy] = 2 A / den
                    const float inv = 1.f / den;
                    dA = 2.f * inv * (mu2 * (Bn - A) + mu1 * (A * Bn) * (1.f / D - 1.f / Cd));
                    dB = -S / D;
                    dC = 2.f * A * inv;
                }
                const uint64_t e = ((uint64_t)b * g.C + c) * plane + (uint64_t)oh * g.W + ow;
                const uint64_t n = (uint64_t)g.B * g.C * plane;
                a.maps[e] = dA;
                a.maps[n + e] = dB;
                a.maps[2 * n + e] = dC;
            }
        }
        __syncthreads();  // the staged tiles are overwritten by the next channel
    }
    const double2 sum = block_sum_f64(make_double2(acc_s, acc_l), s_red);
    if (tid == 0) {
        const uint64_t blk = ((uint64_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        a.partials[2 * blk] = sum.x;
        a.partials[2 * blk + 1] = sum.y;
    }
}

// one block: the partials in a fixed order (thread t takes t, t + 1024, ...; then a fixed tree), the means and the weighted loss
__global__ void __launch_bounds__(SSIM_RED_THREADS) ssim_reduce_kernel(const double *partials, uint32_t n, double inv_s, double inv_l,
                                                                       float lam, float *out_ssim, float *out_l1, float *out_loss) {
    __shared__ double2 s_red[SSIM_RED_THREADS / GS_WAVE];  // (ssim, l1)
    const uint32_t tid = threadIdx.x;
    double s = 0.0, l = 0.0;
    for (uint32_t i = tid; i < n; i += SSIM_RED_THREADS) {
        s += partials[2 * i];
        l += partials[2 * i + 1];
    }
    const double2 sum = block_sum_f64(make_double2(s, l), s_red);
    if (tid == 0) {
        const float ssim = (float)(sum.x * inv_s), l1 = (float)(sum.y * inv_l);
        if (out_ssim) *out_ssim = ssim;
        if (out_l1) *out_l1 = l1;
        if (out_loss) *out_loss = l1 * (1.f - lam) + (1.f - ssim) * lam;
    }
}

struct SsimBwdArgs {
    Geo g;
    Window win;
    const float *maps;
    const float *grad_ssim, *grad_l1;
    float w_ssim, w_l1;
    float inv_s, inv_l;  // 1 / count of the averaged SSIM positions, 1 / B C H W
    float *dx;
    int64_t ds[4];
};

__global__ void __launch_bounds__(GS_BLOCK) ssim_bwd_kernel(SsimBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float s_m[3][SSIM_HR * SSIM_PITCH];
    __shared__ __attribute__((aligned(16))) float s_h[3][SSIM_HR * SSIM_TW];
    const Geo &g = a.g;
    const uint32_t b = blockIdx.z;
    const int32_t h0 = (int32_t)(blockIdx.y * SSIM_TH), w0 = (int32_t)(blockIdx.x * SSIM_TW);
    const uint32_t tid = threadIdx.x;
    const uint32_t col = tid % SSIM_TW, rg = tid / SSIM_TW;
    const uint64_t plane = (uint64_t)g.H * g.W, n = (uint64_t)g.B * g.C * plane;
    const int64_t ms[4] = {(int64_t)g.C * (int64_t)plane, (int64_t)plane, (int64_t)g.W, 1};
    const float gs = a.grad_ssim ? a.w_ssim * a.grad_ssim[0] * a.inv_s : 0.f;
    const float gl = a.grad_l1 ? a.w_l1 * a.grad_l1[0] * a.inv_l : 0.f;
    for (uint32_t c = 0; c < g.C; ++c) {
#pragma unroll
        for (int m = 0; m < 3; ++m) stage(s_m[m], a.maps + m * n, ms, b, c, h0, w0, g.H, g.W);
        __syncthreads();
        for (uint32_t j = tid; j < SSIM_HR * (SSIM_TW / 4); j += GS_BLOCK) {
            const uint32_t r = j / (SSIM_TW / 4), grp = j % (SSIM_TW / 4);
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                float v[16];
                row14(s_m[m] + r * SSIM_PITCH, grp, v);
                float o[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float s = 0.f;
#pragma unroll
                    for (int t = 0; t < 11; ++t) s += a.win.w[t] * v[k + t];
                    o[k] = s;
                }
                *reinterpret_cast<float4 *>(&s_h[m][r * SSIM_TW + 4 * grp]) = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
        __syncthreads();
        float cv[3][4];
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            float v[14];
#pragma unroll
            for (int i = 0; i < 14; ++i) v[i] = s_h[m][(4 * rg + i) * SSIM_TW + col];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float s = 0.f;
#pragma unroll
                for (int t = 0; t < 11; ++t) s += a.win.w[t] * v[k + t];
                cv[m][k] = s;
            }
        }
        const uint32_t ow = (uint32_t)w0 + col;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t oh = (uint32_t)h0 + 4 * rg + k;
            if (oh >= g.H || ow >= g.W) continue;
            const float xc = g.x[(int64_t)b * g.xs[0] + (int64_t)c * g.xs[1] + (int64_t)oh * g.xs[2] + (int64_t)ow * g.xs[3]];
            const float yc = g.y[(int64_t)b * g.ys[0] + (int64_t)c * g.ys[1] + (int64_t)oh * g.ys[2] + (int64_t)ow * g.ys[3]];
            const float d = xc - yc;
            const float sgn = d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f;
            const float v = gs * (cv[0][k] + 2.f * xc * cv[1][k] + yc * cv[2][k]) + gl * sgn;
            a.dx[(int64_t)b * a.ds[0] + (int64_t)c * a.ds[1] + (int64_t)oh * a.ds[2] + (int64_t)ow * a.ds[3]] = v;
        }
        __syncthreads();
    }
}

struct Shape {
    uint32_t tx, ty, blocks;
    uint64_t n, partial_bytes, map_off;
};

Shape shape_of(uint32_t B, uint32_t C, uint32_t H, uint32_t W) {
    Shape s;
    s.tx = gs_div_up(W, SSIM_TW);
    s.ty = gs_div_up(H, SSIM_TH);
    s.blocks = s.tx * s.ty * B;
    s.n = (uint64_t)B * C * H * W;
    s.partial_bytes = 2ull * sizeof(double) * s.blocks;
    s.map_off = (s.partial_bytes + 255) / 256 * 256;
    return s;
}

int32_t check_shape(const char *fn, uint32_t B, uint32_t C, uint32_t H, uint32_t W, int32_t padding) {
    if (B == 0 || C == 0 || H == 0 || W == 0) {
        gs_set_error("%s: empty shape [%u, %u, %u, %u]", fn, B, C, H, W);
        return 1;
    }
    if ((uint64_t)B * C * H * W > 0x7fffffffull) {
        gs_set_error("%s: [%u, %u, %u, %u] has more than 2^31 - 1 elements", fn, B, C, H, W);
        return 1;
    }
    if (B > 65535u) {
        gs_set_error("%s: at most 65535 images per call (B = %u)", fn, B);
        return 1;
    }
    if (padding != GS_SSIM_SAME && padding != GS_SSIM_VALID) {
        gs_set_error("%s: unknown padding %d", fn, padding);
        return 1;
    }
    if (padding == GS_SSIM_VALID && (H <= 10 || W <= 10)) {
        gs_set_error("%s: valid padding needs H > 10 and W > 10 (got %u x %u)", fn, H, W);
        return 1;
    }
    return 0;
}

Geo geo_of(const float *x, const int64_t *xs, const float *y, const int64_t *ys, uint32_t B, uint32_t C, uint32_t H, uint32_t W,
           int32_t padding) {
    Geo g;
    g.x = x;
    g.y = y;
    for (int i = 0; i < 4; ++i) {
        g.xs[i] = xs[i];
        g.ys[i] = ys[i];
    }
    g.B = B;
    g.C = C;
    g.H = H;
    g.W = W;
    g.valid = padding == GS_SSIM_VALID;
    return g;
}

uint64_t averaged_count(uint32_t B, uint32_t C, uint32_t H, uint32_t W, int32_t padding) {
    return padding == GS_SSIM_VALID ? (uint64_t)B * C * (H - 10) * (W - 10) : (uint64_t)B * C * H * W;
}

}  // namespace

extern "C" uint32_t gs_ssim_window(float *out, uint32_t n) {
    const Window w = make_window();
    for (uint32_t i = 0; out != nullptr && i < n && i < 11; ++i) out[i] = w.w[i];
    return 11;
}

extern "C" uint64_t gs_ssim_work_bytes(uint32_t B, uint32_t C, uint32_t H, uint32_t W, int32_t train) {
    const Shape s = shape_of(B, C, H, W);
    return train ? s.map_off + 3ull * sizeof(float) * s.n : s.partial_bytes;
}

extern "C" int32_t gs_ssim_fwd(const float *x, const int64_t *x_strides, const float *y, const int64_t *y_strides, uint32_t B,
                               uint32_t C, uint32_t H, uint32_t W, int32_t padding, int32_t train, float ssim_lambda, void *work,
                               uint64_t work_bytes, float *out_ssim, float *out_l1, float *out_loss, gs_stream_t stream) {
    GS_CHECK_ARG(x && y && x_strides && y_strides && work, "null pointer (x, y, their strides and work are required)");
    GS_CHECK_ARG(out_ssim || out_l1 || out_loss, "null pointer: no output (out_ssim, out_l1, out_loss all null)");
    if (check_shape("gs_ssim_fwd", B, C, H, W, padding)) return 1;
    const Shape s = shape_of(B, C, H, W);
    if (work_bytes < gs_ssim_work_bytes(B, C, H, W, train)) {
        gs_set_error("gs_ssim_fwd: work area of %llu bytes, %llu needed", (unsigned long long)work_bytes,
                     (unsigned long long)gs_ssim_work_bytes(B, C, H, W, train));
        return 1;
    }
    GS_CHECK_ARG((uintptr_t)work % 16 == 0, "work must be 16-byte aligned");
    GS_CHECK_ARG(((uintptr_t)x | (uintptr_t)y) % 4 == 0, "x and y must be 4-byte aligned");
    SsimFwdArgs a;
    a.g = geo_of(x, x_strides, y, y_strides, B, C, H, W, padding);
    a.win = make_window();
    a.train = train ? 1u : 0u;
    a.partials = (double *)work;
    a.maps = train ? (float *)((char *)work + s.map_off) : nullptr;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ssim_fwd_kernel, dim3(s.tx, s.ty, B), dim3(GS_BLOCK), 0, st, a);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(ssim_reduce_kernel, dim3(1), dim3(SSIM_RED_THREADS), 0, st, (const double *)work, s.blocks,
                       1.0 / (double)averaged_count(B, C, H, W, padding), 1.0 / (double)s.n, ssim_lambda, out_ssim, out_l1, out_loss);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_ssim_bwd(const float *x, const int64_t *x_strides, const float *y, const int64_t *y_strides, uint32_t B,
                               uint32_t C, uint32_t H, uint32_t W, int32_t padding, const void *work, uint64_t work_bytes,
                               const float *grad_ssim, float w_ssim, const float *grad_l1, float w_l1, float *dx,
                               const int64_t *dx_strides, gs_stream_t stream) {
    GS_CHECK_ARG(x && y && x_strides && y_strides && work && dx && dx_strides, "null pointer (x, y, work, dx and the strides are required)");
    GS_CHECK_ARG(grad_ssim || w_ssim == 0.f, "null pointer: grad_ssim is required when w_ssim != 0");
    GS_CHECK_ARG(grad_l1 || w_l1 == 0.f, "null pointer: grad_l1 is required when w_l1 != 0");
    if (check_shape("gs_ssim_bwd", B, C, H, W, padding)) return 1;
    const Shape s = shape_of(B, C, H, W);
    if (work_bytes < gs_ssim_work_bytes(B, C, H, W, 1)) {
        gs_set_error("gs_ssim_bwd: work area of %llu bytes, %llu needed (the area of a train forward)", (unsigned long long)work_bytes,
                     (unsigned long long)gs_ssim_work_bytes(B, C, H, W, 1));
        return 1;
    }
    GS_CHECK_ARG((uintptr_t)work % 16 == 0, "work must be 16-byte aligned");
    GS_CHECK_ARG(((uintptr_t)x | (uintptr_t)y | (uintptr_t)dx) % 4 == 0, "x, y and dx must be 4-byte aligned");
    SsimBwdArgs a;
    a.g = geo_of(x, x_strides, y, y_strides, B, C, H, W, padding);
    a.win = make_window();
    a.maps = (const float *)((const char *)work + s.map_off);
    a.grad_ssim = w_ssim != 0.f ? grad_ssim : nullptr;
    a.grad_l1 = w_l1 != 0.f ? grad_l1 : nullptr;
    a.w_ssim = w_ssim;
    a.w_l1 = w_l1;
    a.inv_s = (float)(1.0 / (double)averaged_count(B, C, H, W, padding));
    a.inv_l = (float)(1.0 / (double)s.n);
    a.dx = dx;
    for (int i = 0; i < 4; ++i) a.ds[i] = dx_strides[i];
    hipLaunchKernelGGL(ssim_bwd_kernel, dim3(s.tx, s.ty, B), dim3(GS_BLOCK), 0, (hipStream_t)stream, a);
    GS_CHECK_LAUNCH();
    return 0;
}
