// bilagrid.hip -- the trainers' bilateral-grid colour correction (examples/lib_bilagrid.py: slice, BilateralGrid.forward,
// total_variation_loss), forward and backward (gs_bilagrid_slice_fwd / _bwd, gs_bilagrid_tv_fwd / _bwd).
//
// Slice.  Points are a logical [B, D1, D2] array (an image batch [B, Himg, Wimg]; rays [B, 1, P] or [B, 1, 1]); entry b reads grid
// grid_idx[b] (device memory, clamped to [0, N)).  Per point: x, y from an explicit strided xy tensor (a b stride of 0 broadcasts
// one coordinate image over the batch) or, with xy == NULL, the pixel centre ((j + 0.5) / D2, (i + 0.5) / D1); the guidance
// z = 2 (0.299 r + 0.587 g + 0.114 b) - 1; F.grid_sample's align_corners=True / padding_mode="border" coordinates
// ((c + 1) / 2 * (size - 1), clamped to [0, size - 1]); 12 trilinear values A (row-major 3x4); rgb_out = A[:, :3] rgb + A[:, 3].
// Forward: one thread per point, 96 grid reads (served by L1 / L2: a grid is 12 L H W floats, 96 KB by default), 12 B read and
// 12 B written per point.
//
// Backward.  With g[4 r + c] = v_rgb_out[r] * (rgb, 1)[c] + v_affine[4 r + c]:
//   v_grids[n, k, corner] += w_corner * g[k]                                    (8 corners x 12 values per point)
//   v_rgb[c] = sum_r A[r][c] v_rgb_out[r] + (sum_k dA[k]/dz g[k]) (L - 1) gray[c], the second term 0 where z was clamped.
// torch's grid_sample backward issues the 96 adds per point as global float atomics into the 96 KB grid: 2 10^8 contended atomics
// for one 1080p image.  Here a workgroup owns a tile of BG_TILE points of one batch entry (64 x 32 pixels of an image), finds the
// box of xy cells its points touch (2 x 2 .. 3 x 3 corners at 1080p with a 16 x 16 grid), and accumulates in LDS: box x L x 12
// floats (1.5 - 3.4 KB), kept in up to BG_MAX_REP copies chosen by lane so that neighbouring pixels -- which share their cell --
// do not serialise on one LDS address.  The copies are summed and the non-zero entries added to v_grids with ONE global atomic
// each per workgroup: ~1000 workgroups x <= 864 floats at 1080p, ~2 MB of added bytes against 800 MB for the per-point form.
// The global atomics that remain make v_grids depend on arrival order in its last bits; v_rgb is bit-identical from run to run.
// A tile whose box does not fit the LDS area (BG_LDS_FLOATS) adds to global memory directly, and so does the one-thread-per-point
// kernel used when an entry has fewer than GS_BLOCK points (a ray batch [B, 2]): every shape works, those two paths at the
// atomic rate.
//
// TV.  total_variation_loss of an [N, C, L, H, W] tensor: sum over the three spatial axes of sum (x[i+1] - x[i])^2 / count_axis,
// over N; count_axis = elements per batch entry of the differenced tensor (at least 1; an axis of size 1 contributes 0).  One pass:
// every element takes its three forward differences, squares in float, sums in double; per-block partials and a one-block
// reduction in a fixed order (no atomics, bit-identical from run to run).  Backward: a gather over the <= 6 neighbours.
#include "gs_common.h"

#define BG_PTS 8                        // points per thread of the tiled backward
#define BG_TILE (GS_BLOCK * BG_PTS)     // 2048 points per workgroup
#define BG_TILE_W 64                    // tile of an image: 64 x 32 pixels
#define BG_LDS_FLOATS 8192              // 32 KB accumulation area
#define BG_MAX_REP 8
#define TV_BLOCKS 1024

namespace {

struct SliceGeo {
    const float *grids;  // [N, 12, L, H, W]
    uint32_t N, L, H, W;
    uint32_t B, D1, D2;
    const float *xy;     // null: pixel centres
    int64_t xys[4];      // element strides along b, i, j, component
    const float *rgb;
    int64_t rs[4];
    const int64_t *idx;  // null: entry b reads grid min(b, N - 1)
    int64_t idx_stride;
};

struct Axis {
    uint32_t i0, i1;
    float t;
    bool inside;  // the coordinate was not clamped: its gradient passes
};

// F.grid_sample's unnormalise (align_corners=True) + clip (border) for a coordinate in [-1, 1]; NaN lands on 0
GS_DEV Axis axis_of(float c, uint32_t size) {
    const float top = (float)(size - 1);
    const float u = (c + 1.f) * 0.5f * top;
    const float v = fminf(fmaxf(u, 0.f), top);
    Axis a;
    a.inside = u > 0.f && u < top;
    if (size > 1) {
        a.i0 = min((uint32_t)v, size - 2);
        a.i1 = a.i0 + 1;
        a.t = v - (float)a.i0;
    } else {
        a.i0 = a.i1 = 0;
        a.t = 0.f;
    }
    return a;
}

GS_DEV void xy_axes(const SliceGeo &g, uint32_t b, uint32_t i, uint32_t j, Axis &ax, Axis &ay) {
    float x, y;
    if (g.xy) {
        const float *p = g.xy + (int64_t)b * g.xys[0] + (int64_t)i * g.xys[1] + (int64_t)j * g.xys[2];
        x = p[0];
        y = p[g.xys[3]];
    } else {
        x = ((float)j + 0.5f) / (float)g.D2;
        y = ((float)i + 0.5f) / (float)g.D1;
    }
    ax = axis_of((x - 0.5f) * 2.f, g.W);
    ay = axis_of((y - 0.5f) * 2.f, g.H);
}

GS_DEV void load_rgb(const SliceGeo &g, uint32_t b, uint32_t i, uint32_t j, float c[3]) {
    const float *p = g.rgb + (int64_t)b * g.rs[0] + (int64_t)i * g.rs[1] + (int64_t)j * g.rs[2];
    c[0] = p[0];
    c[1] = p[g.rs[3]];
    c[2] = p[2 * g.rs[3]];
}

// The guidance axis.  The cell a point falls into is a discontinuity of its colour gradient (dA/dz is constant per cell), so the
// cell and the clamp test are evaluated in double: a float32 evaluation puts the few points that lie within a rounding error of
// a cell border into the neighbouring cell, each with an O(1) error in v_rgb.  (x and y need no such care: nothing is
// differentiated with respect to them, and the interpolated values are continuous across cells.)
GS_DEV Axis z_axis(const SliceGeo &g, const float c[3]) {
    const double top = (double)(g.L - 1);
    const double z = (0.299 * (double)c[0] + 0.587 * (double)c[1] + 0.114 * (double)c[2]) * 2.0 - 1.0;
    const double u = (z + 1.0) * 0.5 * top;
    const double v = fmin(fmax(u, 0.0), top);
    Axis a;
    a.inside = u > 0.0 && u < top;
    if (g.L > 1) {
        a.i0 = min((uint32_t)v, g.L - 2);
        a.i1 = a.i0 + 1;
        a.t = (float)(v - (double)a.i0);
    } else {
        a.i0 = a.i1 = 0;
        a.t = 0.f;
    }
    return a;
}

GS_DEV const float *grid_of(const SliceGeo &g, uint32_t b, uint32_t &n) {
    int64_t v = g.idx ? g.idx[(int64_t)b * g.idx_stride] : (int64_t)b;
    v = v < 0 ? 0 : v > (int64_t)g.N - 1 ? (int64_t)g.N - 1 : v;
    n = (uint32_t)v;
    return g.grids + (size_t)n * 12u * g.L * g.H * g.W;
}

struct Corners {
    uint32_t off[8];  // inside one channel of one grid: bit 2 z, bit 1 y, bit 0 x
    float w[8];
    float wxy[4];
};

GS_DEV Corners corners_of(const SliceGeo &g, const Axis &ax, const Axis &ay, const Axis &az) {
    Corners c;
    const float wx[2] = {1.f - ax.t, ax.t}, wy[2] = {1.f - ay.t, ay.t}, wz[2] = {1.f - az.t, az.t};
    const uint32_t xs[2] = {ax.i0, ax.i1}, ys[2] = {ay.i0, ay.i1}, zs[2] = {az.i0, az.i1};
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int dz = q >> 2, dy = (q >> 1) & 1, dx = q & 1;
        c.off[q] = (zs[dz] * g.H + ys[dy]) * g.W + xs[dx];
        c.w[q] = wz[dz] * wy[dy] * wx[dx];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) c.wxy[q] = wy[q >> 1] * wx[q & 1];
    return c;
}

struct SliceFwdArgs {
    SliceGeo g;
    float *out_rgb;  // [B, D1, D2, 3] or null
    float *out_aff;  // [B, D1, D2, 12] or null
};

__global__ void __launch_bounds__(GS_BLOCK) bilagrid_slice_fwd_kernel(SliceFwdArgs a) {
    const SliceGeo &g = a.g;
    const uint32_t P = g.D1 * g.D2;
    const uint32_t q = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (q >= g.B * P) return;
    const uint32_t b = q / P, p = q - b * P, i = p / g.D2, j = p - i * g.D2;
    Axis ax, ay;
    xy_axes(g, b, i, j, ax, ay);
    float c[3];
    load_rgb(g, b, i, j, c);
    const Axis az = z_axis(g, c);
    const Corners cn = corners_of(g, ax, ay, az);
    uint32_t n;
    const float *grid = grid_of(g, b, n);
    const uint32_t chan = g.L * g.H * g.W;
    float A[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const float *gk = grid + (size_t)k * chan;
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) s += cn.w[r] * gk[cn.off[r]];
        A[k] = s;
    }
    if (a.out_rgb) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
            a.out_rgb[(size_t)q * 3 + r] = A[4 * r] * c[0] + A[4 * r + 1] * c[1] + A[4 * r + 2] * c[2] + A[4 * r + 3];
    }
    if (a.out_aff) {
        float4 *o = reinterpret_cast<float4 *>(a.out_aff + (size_t)q * 12);
        o[0] = make_float4(A[0], A[1], A[2], A[3]);
        o[1] = make_float4(A[4], A[5], A[6], A[7]);
        o[2] = make_float4(A[8], A[9], A[10], A[11]);
    }
}

struct SliceBwdArgs {
    SliceGeo g;
    const float *v_out;  // [B, D1, D2, 3] or null
    const float *v_aff;  // [B, D1, D2, 12] or null
    float *v_grids;      // [N, 12, L, H, W] (zeroed by the entry point) or null
    float *v_rgb;        // [B, D1, D2, 3] or null
    uint32_t tw, th;     // tile of the tiled kernel: tw * th == BG_TILE
    uint32_t ntx, nty;
};

// LDS: acc points into the workgroup's shared array (an LDS atomic), otherwise into global memory
template <bool LDS>
GS_DEV void point_bwd(const SliceBwdArgs &a, const float *grid, uint32_t b, uint32_t i, uint32_t j, const Axis &ax, const Axis &ay,
                      float *acc_base, uint32_t acc_chan, uint32_t bx0, uint32_t by0, uint32_t nx, uint32_t ny, bool want_grid) {
    const SliceGeo &g = a.g;
    const size_t q = ((size_t)b * g.D1 + i) * g.D2 + j;
    float c[3];
    load_rgb(g, b, i, j, c);
    const Axis az = z_axis(g, c);
    const Corners cn = corners_of(g, ax, ay, az);
    const uint32_t chan = g.L * g.H * g.W;
    uint32_t aoff[8];
    if (LDS) {
        // inside the box by construction (the box is the extent of these same cells); the min keeps a write inside LDS regardless
        const uint32_t xs[2] = {min(ax.i0 - bx0, nx - 1), min(ax.i1 - bx0, nx - 1)};
        const uint32_t ys[2] = {min(ay.i0 - by0, ny - 1), min(ay.i1 - by0, ny - 1)}, zs[2] = {az.i0, az.i1};
#pragma unroll
        for (int s = 0; s < 8; ++s) aoff[s] = (zs[s >> 2] * ny + ys[(s >> 1) & 1]) * nx + xs[s & 1];
    } else {
#pragma unroll
        for (int s = 0; s < 8; ++s) aoff[s] = cn.off[s];
    }
    float vo[3] = {0.f, 0.f, 0.f};
    if (a.v_out) {
        vo[0] = a.v_out[q * 3];
        vo[1] = a.v_out[q * 3 + 1];
        vo[2] = a.v_out[q * 3 + 2];
    }
    const float h[4] = {c[0], c[1], c[2], 1.f};
    float vrgb[3] = {0.f, 0.f, 0.f};
    float gz = 0.f;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const int r = k >> 2, cc = k & 3;
        float gk = vo[r] * h[cc];
        if (a.v_aff) gk += a.v_aff[q * 12 + k];
        const float *p = grid + (size_t)k * chan;
        float v[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) v[s] = p[cn.off[s]];
        float daz = 0.f;
#pragma unroll
        for (int s = 0; s < 4; ++s) daz += cn.wxy[s] * (v[4 + s] - v[s]);
        gz += daz * gk;
        if (cc < 3) {
            float ak = 0.f;
#pragma unroll
            for (int s = 0; s < 8; ++s) ak += cn.w[s] * v[s];
            vrgb[cc] += ak * vo[r];
        }
        if (want_grid) {
#pragma unroll
            for (int s = 0; s < 8; ++s) atomicAdd(acc_base + (size_t)k * acc_chan + aoff[s], cn.w[s] * gk);
        }
    }
    if (a.v_rgb) {
        const float gzs = az.inside ? gz * (float)(g.L - 1) : 0.f;
        a.v_rgb[q * 3] = vrgb[0] + gzs * 0.299f;
        a.v_rgb[q * 3 + 1] = vrgb[1] + gzs * 0.587f;
        a.v_rgb[q * 3 + 2] = vrgb[2] + gzs * 0.114f;
    }
}

__global__ void __launch_bounds__(GS_BLOCK) bilagrid_slice_bwd_tiled_kernel(SliceBwdArgs a) {
    __shared__ float s_acc[BG_LDS_FLOATS];
    __shared__ uint32_t s_box[4];  // x min, x max, y min, y max over the corners the tile touches
    const SliceGeo &g = a.g;
    const uint32_t tid = threadIdx.x;
    const uint32_t tiles = a.ntx * a.nty;
    const uint32_t b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
    const uint32_t i0 = (t / a.ntx) * a.th, j0 = (t % a.ntx) * a.tw;
    uint32_t n;
    const float *grid = grid_of(g, b, n);
    const bool want_grid = a.v_grids != nullptr;

    uint32_t bx0 = g.W, bx1 = 0, by0 = g.H, by1 = 0;
    if (tid == 0) {
        s_box[0] = g.W;
        s_box[1] = 0;
        s_box[2] = g.H;
        s_box[3] = 0;
    }
#pragma unroll
    for (int s = 0; s < BG_PTS; ++s) {
        const uint32_t q = tid + s * GS_BLOCK, i = i0 + q / a.tw, j = j0 + q % a.tw;
        if (want_grid && i < g.D1 && j < g.D2) {
            Axis ax, ay;
            xy_axes(g, b, i, j, ax, ay);
            bx0 = min(bx0, ax.i0);
            bx1 = max(bx1, ax.i1);
            by0 = min(by0, ay.i0);
            by1 = max(by1, ay.i1);
        }
    }
    uint32_t nx = 0, ny = 0, stride = 0, reps = 0;
    if (want_grid) {
        bx0 = wave_min_u32(bx0);
        bx1 = wave_max_u32(bx1);
        by0 = wave_min_u32(by0);
        by1 = wave_max_u32(by1);
        __syncthreads();
        if (lane_id() == 0) {
            atomicMin(&s_box[0], bx0);
            atomicMax(&s_box[1], bx1);
            atomicMin(&s_box[2], by0);
            atomicMax(&s_box[3], by1);
        }
        __syncthreads();
        bx0 = s_box[0];
        bx1 = s_box[1];
        by0 = s_box[2];
        by1 = s_box[3];
        if (bx0 > bx1 || by0 > by1) return;  // no point of this tile is inside [B, D1, D2] (cannot happen for a launched tile)
        nx = bx1 - bx0 + 1;
        ny = by1 - by0 + 1;
        const uint64_t box = 12ull * g.L * ny * nx;
        // copies one float past a multiple of 32 apart: the same entry of different copies sits in different LDS banks
        if (box <= BG_LDS_FLOATS) {
            stride = ((uint32_t)box + 31u) / 32u * 32u + 1u;
            reps = min((uint32_t)BG_MAX_REP, (uint32_t)BG_LDS_FLOATS / stride);
            if (reps == 0) {
                stride = (uint32_t)box;
                reps = 1;
            }
            for (uint32_t e = tid; e < reps * stride; e += GS_BLOCK) s_acc[e] = 0.f;
        }
        __syncthreads();
    }
    const uint32_t chan = g.L * g.H * g.W;
    float *const grid_acc = want_grid ? a.v_grids + (size_t)n * 12u * chan : nullptr;
    float *const lds_acc = s_acc + (reps ? (tid % reps) * stride : 0u);
#pragma unroll 1
    for (int s = 0; s < BG_PTS; ++s) {
        const uint32_t q = tid + s * GS_BLOCK, i = i0 + q / a.tw, j = j0 + q % a.tw;
        if (i >= g.D1 || j >= g.D2) continue;
        Axis ax, ay;
        xy_axes(g, b, i, j, ax, ay);  // as in the first pass: the same cells
        if (reps)
            point_bwd<true>(a, grid, b, i, j, ax, ay, lds_acc, g.L * ny * nx, bx0, by0, nx, ny, want_grid);
        else
            point_bwd<false>(a, grid, b, i, j, ax, ay, grid_acc, chan, 0, 0, 0, 0, want_grid);
    }
    if (!reps) return;
    __syncthreads();
    const uint32_t box = 12u * g.L * ny * nx;
    for (uint32_t e = tid; e < box; e += GS_BLOCK) {
        float v = 0.f;
        for (uint32_t r = 0; r < reps; ++r) v += s_acc[r * stride + e];
        if (v != 0.f) {
            const uint32_t x = e % nx, r1 = e / nx, y = r1 % ny, kz = r1 / ny;  // kz = k * L + z
            atomicAdd(grid_acc + ((size_t)kz * g.H + (by0 + y)) * g.W + (bx0 + x), v);
        }
    }
}

__global__ void __launch_bounds__(GS_BLOCK) bilagrid_slice_bwd_point_kernel(SliceBwdArgs a) {
    const SliceGeo &g = a.g;
    const uint32_t P = g.D1 * g.D2;
    const uint32_t q = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (q >= g.B * P) return;
    const uint32_t b = q / P, p = q - b * P, i = p / g.D2, j = p - i * g.D2;
    uint32_t n;
    const float *grid = grid_of(g, b, n);
    Axis ax, ay;
    xy_axes(g, b, i, j, ax, ay);
    const uint32_t chan = g.L * g.H * g.W;
    const bool want_grid = a.v_grids != nullptr;
    point_bwd<false>(a, grid, b, i, j, ax, ay, want_grid ? a.v_grids + (size_t)n * 12u * chan : nullptr, chan, 0, 0, 0, 0, want_grid);
}

// ---------------------------------------------------------------------------------------------------------------- TV
struct TvGeo {
    uint32_t n, L, H, W;  // n = N C L H W
    double cl, ch, cw;    // 1 / (count_axis N); 0 for an axis of size 1
};

__global__ void __launch_bounds__(GS_BLOCK) bilagrid_tv_fwd_kernel(const float *x, TvGeo g, double *partials) {
    __shared__ double s_red[GS_BLOCK / GS_WAVE];
    const uint32_t hw = g.H * g.W;
    double acc = 0.0;
    for (uint32_t e = blockIdx.x * GS_BLOCK + threadIdx.x; e < g.n; e += gridDim.x * GS_BLOCK) {
        const uint32_t w = e % g.W, h = (e / g.W) % g.H, l = (e / hw) % g.L;
        const float v = x[e];
        if (w + 1 < g.W) {
            const float d = x[e + 1] - v;
            acc += (double)(d * d) * g.cw;
        }
        if (h + 1 < g.H) {
            const float d = x[e + g.W] - v;
            acc += (double)(d * d) * g.ch;
        }
        if (l + 1 < g.L) {
            const float d = x[e + hw] - v;
            acc += (double)(d * d) * g.cl;
        }
    }
    acc = block_sum_f64(acc, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(GS_BLOCK) bilagrid_tv_reduce_kernel(const double *partials, uint32_t n, float *out) {
    __shared__ double s_red[GS_BLOCK / GS_WAVE];
    double s = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += GS_BLOCK) s += partials[i];
    s = block_sum_f64(s, s_red);
    if (threadIdx.x == 0) *out = (float)s;
}

__global__ void __launch_bounds__(GS_BLOCK) bilagrid_tv_bwd_kernel(const float *x, TvGeo g, const float *grad, float *v_x) {
    const uint32_t e = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (e >= g.n) return;
    const uint32_t hw = g.H * g.W;
    const uint32_t w = e % g.W, h = (e / g.W) % g.H, l = (e / hw) % g.L;
    const float v = x[e];
    const float cw = (float)(2.0 * g.cw), ch = (float)(2.0 * g.ch), cl = (float)(2.0 * g.cl);
    float s = 0.f;
    if (w > 0) s += cw * (v - x[e - 1]);
    if (w + 1 < g.W) s -= cw * (x[e + 1] - v);
    if (h > 0) s += ch * (v - x[e - g.W]);
    if (h + 1 < g.H) s -= ch * (x[e + g.W] - v);
    if (l > 0) s += cl * (v - x[e - hw]);
    if (l + 1 < g.L) s -= cl * (x[e + hw] - v);
    v_x[e] = grad[0] * s;
}

int32_t slice_geo(const char *fn, SliceGeo &g, const float *grids, uint32_t N, uint32_t L, uint32_t H, uint32_t W, uint32_t B,
                  uint32_t D1, uint32_t D2, const float *xy, const int64_t *xy_strides, const float *rgb, const int64_t *rgb_strides,
                  const int64_t *grid_idx, int64_t idx_stride) {
    if (!grids || !rgb || !rgb_strides) {
        gs_set_error("%s: null pointer (grids, rgb and rgb_strides are required)", fn);
        return 1;
    }
    if (xy && !xy_strides) {
        gs_set_error("%s: null pointer (xy_strides is required with xy)", fn);
        return 1;
    }
    if (N == 0 || L == 0 || H == 0 || W == 0) {
        gs_set_error("%s: empty grid shape [%u, 12, %u, %u, %u]", fn, N, L, H, W);
        return 1;
    }
    if (12ull * L * H * W > 0x7fffffffull) {
        gs_set_error("%s: a grid of [12, %u, %u, %u] has more than 2^31 - 1 elements", fn, L, H, W);
        return 1;
    }
    if (B == 0 || D1 == 0 || D2 == 0) {
        gs_set_error("%s: empty point shape [%u, %u, %u]", fn, B, D1, D2);
        return 1;
    }
    if ((uint64_t)B * D1 * D2 > 0x7fffffffull) {
        gs_set_error("%s: [%u, %u, %u] has more than 2^31 - 1 points", fn, B, D1, D2);
        return 1;
    }
    if ((((uintptr_t)grids | (uintptr_t)rgb | (uintptr_t)xy) % 4) != 0 || ((uintptr_t)grid_idx % 8) != 0) {
        gs_set_error("%s: misaligned pointer (floats need 4-byte, grid_idx 8-byte alignment)", fn);
        return 1;
    }
    g.grids = grids;
    g.N = N;
    g.L = L;
    g.H = H;
    g.W = W;
    g.B = B;
    g.D1 = D1;
    g.D2 = D2;
    g.xy = xy;
    g.rgb = rgb;
    for (int i = 0; i < 4; ++i) {
        g.xys[i] = xy ? xy_strides[i] : 0;
        g.rs[i] = rgb_strides[i];
    }
    g.idx = grid_idx;
    g.idx_stride = idx_stride;
    return 0;
}

int32_t tv_geo(const char *fn, TvGeo &g, uint32_t N, uint32_t C, uint32_t L, uint32_t H, uint32_t W) {
    if (N == 0 || C == 0 || L == 0 || H == 0 || W == 0) {
        gs_set_error("%s: empty shape [%u, %u, %u, %u, %u]", fn, N, C, L, H, W);
        return 1;
    }
    const uint64_t per = (uint64_t)C * L * H * W;
    if (per > 0x7fffffffull || per * N > 0x7fffffffull) {
        gs_set_error("%s: [%u, %u, %u, %u, %u] has more than 2^31 - 1 elements", fn, N, C, L, H, W);
        return 1;
    }
    g.n = (uint32_t)(per * N);
    g.L = L;
    g.H = H;
    g.W = W;
    auto coef = [&](uint32_t size) {
        if (size < 2) return 0.0;
        const double count = (double)(per / size) * (double)(size - 1);
        return 1.0 / (count * (double)N);
    };
    g.cl = coef(L);
    g.ch = coef(H);
    g.cw = coef(W);
    return 0;
}

}  // namespace

extern "C" int32_t gs_bilagrid_slice_fwd(const float *grids, uint32_t N, uint32_t L, uint32_t H, uint32_t W, uint32_t B, uint32_t D1,
                                         uint32_t D2, const float *xy, const int64_t *xy_strides, const float *rgb,
                                         const int64_t *rgb_strides, const int64_t *grid_idx, int64_t idx_stride, float *out_rgb,
                                         float *out_affine, gs_stream_t stream) {
    SliceFwdArgs a;
    if (slice_geo("gs_bilagrid_slice_fwd", a.g, grids, N, L, H, W, B, D1, D2, xy, xy_strides, rgb, rgb_strides, grid_idx, idx_stride))
        return 1;
    GS_CHECK_ARG(out_rgb || out_affine, "null pointer: no output (out_rgb and out_affine both null)");
    GS_CHECK_ARG((uintptr_t)out_rgb % 4 == 0 && (uintptr_t)out_affine % 16 == 0, "out_rgb must be 4-byte, out_affine 16-byte aligned");
    a.out_rgb = out_rgb;
    a.out_aff = out_affine;
    hipLaunchKernelGGL(bilagrid_slice_fwd_kernel, dim3(gs_div_up((uint64_t)B * D1 * D2, GS_BLOCK)), dim3(GS_BLOCK), 0,
                       (hipStream_t)stream, a);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_bilagrid_slice_bwd(const float *grids, uint32_t N, uint32_t L, uint32_t H, uint32_t W, uint32_t B, uint32_t D1,
                                         uint32_t D2, const float *xy, const int64_t *xy_strides, const float *rgb,
                                         const int64_t *rgb_strides, const int64_t *grid_idx, int64_t idx_stride,
                                         const float *v_out_rgb, const float *v_out_affine, float *v_grids, float *v_rgb,
                                         gs_stream_t stream) {
    SliceBwdArgs a;
    if (slice_geo("gs_bilagrid_slice_bwd", a.g, grids, N, L, H, W, B, D1, D2, xy, xy_strides, rgb, rgb_strides, grid_idx, idx_stride))
        return 1;
    GS_CHECK_ARG(v_out_rgb || v_out_affine, "null pointer: no upstream gradient (v_out_rgb and v_out_affine both null)");
    GS_CHECK_ARG(v_grids || v_rgb, "null pointer: no output (v_grids and v_rgb both null)");
    GS_CHECK_ARG(((uintptr_t)v_out_rgb | (uintptr_t)v_out_affine | (uintptr_t)v_grids | (uintptr_t)v_rgb) % 4 == 0,
                 "the gradient arrays must be 4-byte aligned");
    a.v_out = v_out_rgb;
    a.v_aff = v_out_affine;
    a.v_grids = v_grids;
    a.v_rgb = v_rgb;
    const hipStream_t st = (hipStream_t)stream;
    if (v_grids) {
        const hipError_t e = hipMemsetAsync(v_grids, 0, sizeof(float) * 12ull * N * L * H * W, st);
        if (e != hipSuccess) {
            gs_set_error("gs_bilagrid_slice_bwd: clearing v_grids failed: %s", hipGetErrorString(e));
            return 2;
        }
    }
    const uint64_t P = (uint64_t)D1 * D2;
    if (P < GS_BLOCK) {
        a.tw = a.th = a.ntx = a.nty = 0;
        hipLaunchKernelGGL(bilagrid_slice_bwd_point_kernel, dim3(gs_div_up((uint64_t)B * P, GS_BLOCK)), dim3(GS_BLOCK), 0, st, a);
        GS_CHECK_LAUNCH();
        return 0;
    }
    // a tile is BG_TILE points: 64 x 32 of an image, one row of a [B, 1, P] batch
    a.tw = D1 >= BG_TILE / BG_TILE_W ? BG_TILE_W : D1 == 1 ? BG_TILE : BG_TILE / 8;
    a.th = BG_TILE / a.tw;
    a.ntx = gs_div_up(D2, a.tw);
    a.nty = gs_div_up(D1, a.th);
    const uint64_t blocks = (uint64_t)B * a.ntx * a.nty;
    if (blocks > 0x7fffffffull) {
        gs_set_error("gs_bilagrid_slice_bwd: [%u, %u, %u] needs %llu workgroups, more than 2^31 - 1", B, D1, D2,
                     (unsigned long long)blocks);
        return 1;
    }
    hipLaunchKernelGGL(bilagrid_slice_bwd_tiled_kernel, dim3((uint32_t)blocks), dim3(GS_BLOCK), 0, st, a);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" uint64_t gs_bilagrid_tv_work_bytes(void) { return sizeof(double) * TV_BLOCKS; }

extern "C" int32_t gs_bilagrid_tv_fwd(const float *x, uint32_t N, uint32_t C, uint32_t L, uint32_t H, uint32_t W, void *work,
                                      uint64_t work_bytes, float *out, gs_stream_t stream) {
    GS_CHECK_ARG(x && work && out, "null pointer (x, work and out are required)");
    TvGeo g;
    if (tv_geo("gs_bilagrid_tv_fwd", g, N, C, L, H, W)) return 1;
    if (work_bytes < gs_bilagrid_tv_work_bytes()) {
        gs_set_error("gs_bilagrid_tv_fwd: work area of %llu bytes, %llu needed", (unsigned long long)work_bytes,
                     (unsigned long long)gs_bilagrid_tv_work_bytes());
        return 1;
    }
    GS_CHECK_ARG((uintptr_t)work % 8 == 0 && ((uintptr_t)x | (uintptr_t)out) % 4 == 0, "work must be 8-byte, x and out 4-byte aligned");
    const uint32_t blocks = min((uint32_t)TV_BLOCKS, gs_div_up(g.n, GS_BLOCK));
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bilagrid_tv_fwd_kernel, dim3(blocks), dim3(GS_BLOCK), 0, st, x, g, (double *)work);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(bilagrid_tv_reduce_kernel, dim3(1), dim3(GS_BLOCK), 0, st, (const double *)work, blocks, out);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_bilagrid_tv_bwd(const float *x, uint32_t N, uint32_t C, uint32_t L, uint32_t H, uint32_t W, const float *grad,
                                      float *v_x, gs_stream_t stream) {
    GS_CHECK_ARG(x && grad && v_x, "null pointer (x, grad and v_x are required)");
    TvGeo g;
    if (tv_geo("gs_bilagrid_tv_bwd", g, N, C, L, H, W)) return 1;
    GS_CHECK_ARG(((uintptr_t)x | (uintptr_t)grad | (uintptr_t)v_x) % 4 == 0, "x, grad and v_x must be 4-byte aligned");
    hipLaunchKernelGGL(bilagrid_tv_bwd_kernel, dim3(gs_div_up(g.n, GS_BLOCK)), dim3(GS_BLOCK), 0, (hipStream_t)stream, x, g, grad, v_x);
    GS_CHECK_LAUNCH();
    return 0;
}
