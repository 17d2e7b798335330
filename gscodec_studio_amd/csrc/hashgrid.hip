// hashgrid.hip -- position-conditioned Gaussian entropy model (the rate term selected by the reference trainer's
// `--entropy_model_type gaussian_model`): multi-resolution hash-grid encoder and Gaussian bits, forward + backward (gfx950).
//
// Replaces the reference's CUDA-only `_gridencoder` extension (third_party/gridencoder, driven by
// gsplat/compression_simulation/gaussian_distribution_model.py) and the torch graph of Entropy_gaussian.forward
// (entropy_model.py:323-339).  What changes against the reference's shape of the work:
//   * ONE launch each way covers every level of up to four grids (xyz, xy, xz, yz) through a level table passed by value;
//     the reference launches once per grid, chunks / concatenates the positions and concatenates the four outputs.
//   * The output is written row-major [N, levels * F] in its final layout (the reference writes [L, N, F] and permutes).
//   * STE_binary is evaluated on the raw parameter inside the kernels: the [rows, F] sign tensor and its mask never exist.
//   * The input gradient is recomputed in the backward: no [N, L * D * F] dy_dx buffer.
//   * v_pos is summed over the levels of a point in LDS in level order by one owner lane: no float atomics, bit-identical
//     from run to run.  The table gradient uses float atomics (scattered rows; -munsafe-fp-atomics).
//
// Mapping: a lane per (point, level), the level fastest: the 256 threads of a workgroup hold 256 / levels whole points, so
// the stores of a workgroup are one contiguous run of the output, the position loads are broadcasts, and the per-point sum of
// the backward stays inside the workgroup.  The tables are a few MB (reference configuration: 441,568 rows x 2 floats): the
// gathers are served by L2, not HBM.  A wave mixes 3-D and 2-D levels; the two bodies run one after the other.
//
// The Gaussian bits are one elementwise kernel each way over x [M, C] and the MLP output net [M, 2C] (means | raw scales).
#include "gs_common.h"

#include <cmath>

namespace {

constexpr uint32_t HG_MAX_GRIDS = 4;
constexpr uint32_t HG_MAX_LEVELS = 32;
constexpr uint32_t HG_AXES_XYZ = 0, HG_AXES_XY = 1; // axis selectors: 0 xyz, 1 xy, 2 xz, 3 yz
constexpr uint32_t HG_MAX_RES = 1u << 24; // float(R - 2) is exact

struct HgLevel {
    const float *table; // first row of the level's slice
    float *v_table;     // same slice of the gradient (nullptr: skipped)
    uint32_t T;         // rows of the slice
    uint32_t R;         // resolution
    uint32_t dims;      // num_dim | axis0 << 4 | axis1 << 8 | axis2 << 12
    uint32_t pad_;
};

struct HgArgs {
    HgLevel lv[HG_MAX_LEVELS];
    uint64_t n;
    uint32_t n_levels, pos_dim, ppb; // ppb: points per workgroup = 256 / n_levels
    const float *pos;
};

// cell and fractional offset of one coordinate: p = u * float(R - 2) + 0.5f in two float32 roundings (no fma: the cell a
// point falls into must not depend on the kernel this is inlined into)
GS_DEV void hg_cell(float u, float r2, uint32_t &g, float &f) {
    GS_FP_STRICT;
    float p = u * r2;
    p = p + 0.5f;
    const float fl = floorf(p);
    g = (uint32_t)fl;
    f = p - fl;
}

template <int D>
GS_DEV uint32_t hg_row(const uint32_t (&c)[D], uint32_t R, uint32_t T) {
    uint32_t stride = 1, index = 0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        if (stride <= T) {
            index += c[d] * stride;
            stride *= R;
        }
    }
    if (stride > T) {
        constexpr uint32_t primes[3] = {1u, 2654435761u, 805459861u};
        index = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) index ^= c[d] * primes[d];
    }
    return index % T;
}

template <int F>
struct HgVec {
    float v[F];
};

template <int F>
GS_DEV HgVec<F> hg_load(const float *p) {
    HgVec<F> r;
    if constexpr (F == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else if constexpr (F == 2) {
        const float2 t = *reinterpret_cast<const float2 *>(p);
        r.v[0] = t.x; r.v[1] = t.y;
    } else {
        r.v[0] = *p;
    }
    return r;
}

template <int F>
GS_DEV void hg_store(float *p, const HgVec<F> &r) {
    if constexpr (F == 4)
        *reinterpret_cast<float4 *>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else if constexpr (F == 2)
        *reinterpret_cast<float2 *>(p) = make_float2(r.v[0], r.v[1]);
    else
        *p = r.v[0];
}

// One (point, level) pair.  Forward: returns the level's F outputs.  Backward: adds the table gradient with atomics and
// returns the gradient of the level's D coordinates in v_u.
template <int D, int F, bool STE, bool BWD>
GS_DEV HgVec<F> hg_level(const HgLevel &lv, const float (&u)[D], const HgVec<F> &v_out, float (&v_u)[D]) {
    constexpr int NC = 1 << D;
    const uint32_t R = lv.R, T = lv.T;
    const float r2 = (float)(R - 2u);
    uint32_t g[D];
    float f[D];
#pragma unroll
    for (int d = 0; d < D; ++d) hg_cell(u[d], r2, g[d], f[d]);

    float w[NC];
    float e[NC][F]; // embedding of each corner, 0 for a border corner
    bool pass[NC][F]; // STE mask of the raw parameter (backward)
    uint32_t row[NC];
    bool live[NC];
    float wn = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        uint32_t c[D];
        float wi = 1.f;
        bool border = false;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (i & (1 << d)) {
                wi *= f[d];
                c[d] = min(g[d] + 1u, R - 1u);
            } else {
                wi *= 1.f - f[d];
                c[d] = g[d];
            }
            border = border || c[d] == 0u || c[d] == R - 1u;
        }
        w[i] = wi;
        live[i] = !border;
        row[i] = 0;
#pragma unroll
        for (int ch = 0; ch < F; ++ch) {
            e[i][ch] = 0.f;
            pass[i][ch] = false;
        }
        if (!border) {
            row[i] = hg_row<D>(c, R, T);
            wn += wi;
            const HgVec<F> raw = hg_load<F>(lv.table + (size_t)row[i] * F);
#pragma unroll
            for (int ch = 0; ch < F; ++ch) {
                const float p = raw.v[ch];
                if (STE) {
                    e[i][ch] = (p >= 0.f ? 1.f : 0.f) - (p < 0.f ? 1.f : 0.f); // +-1, 0 for NaN
                    pass[i][ch] = p >= -1.f && p <= 1.f;
                } else {
                    e[i][ch] = p;
                    pass[i][ch] = true;
                }
            }
        }
    }
    if (wn == 0.f) wn = 1e-9f;
    const float wn_re = 1.f / wn;

    HgVec<F> out;
#pragma unroll
    for (int ch = 0; ch < F; ++ch) out.v[ch] = 0.f;
    if constexpr (!BWD) {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            if (live[i]) {
                const float coef = w[i] * wn_re;
#pragma unroll
                for (int ch = 0; ch < F; ++ch) out.v[ch] += coef * e[i][ch];
            }
        }
        return out;
    } else {
        if (lv.v_table != nullptr) {
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                if (live[i]) {
                    const float coef = w[i] * wn_re;
#pragma unroll
                    for (int ch = 0; ch < F; ++ch) {
                        const float v = coef * v_out.v[ch];
                        if (pass[i][ch] && v != 0.f) unsafeAtomicAdd(lv.v_table + (size_t)row[i] * F + ch, v);
                    }
                }
            }
        }
        // the reference's dy_dx: finite difference of the corner values along gd, weighted by the other axes' weights;
        // a border corner counts as 0 and the renormalisation does not enter
#pragma unroll
        for (int gd = 0; gd < D; ++gd) {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                if (i & (1 << gd)) continue; // i: the pair's left corner
                float wp = r2;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    if (d == gd) continue;
                    wp *= (i & (1 << d)) ? f[d] : 1.f - f[d];
                }
                float s = 0.f;
#pragma unroll
                for (int ch = 0; ch < F; ++ch) s += v_out.v[ch] * (e[i | (1 << gd)][ch] - e[i][ch]);
                acc += wp * s;
            }
            v_u[gd] = acc;
        }
        return out;
    }
}

template <int F, bool STE, bool BWD>
__global__ void __launch_bounds__(256) hashgrid_kernel(HgArgs a, float *__restrict__ out, const float *__restrict__ v_out,
                                                        float *__restrict__ v_pos) {
    __shared__ HgLevel s_lv[HG_MAX_LEVELS];
    __shared__ float s_vu[BWD ? 256 * 3 : 1];
    const uint32_t tid = threadIdx.x;
    const uint32_t L = a.n_levels;
    if (tid == 0) {
        for (uint32_t i = 0; i < L; ++i) s_lv[i] = a.lv[i]; // uniform index: scalar loads of the kernel arguments
    }
    __syncthreads();
    const uint32_t p_local = tid / L, l = tid - p_local * L;
    const uint64_t b = (uint64_t)blockIdx.x * a.ppb + p_local;
    const bool active = p_local < a.ppb && b < a.n;
    float vp[3] = {0.f, 0.f, 0.f}; // this level's share of the point's position gradient
    if (active) {
        const HgLevel lv = s_lv[l];
        const uint32_t D = lv.dims & 0xfu;
        float u[3];
        bool oob = false;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const uint32_t axis = (lv.dims >> (4 + 4 * d)) & 0xfu;
            u[d] = (uint32_t)d < D ? a.pos[b * a.pos_dim + axis] : 0.f;
            oob = oob || !(u[d] >= 0.f && u[d] <= 1.f); // NaN is out of range too
        }
        const size_t o = ((size_t)b * L + l) * F;
        HgVec<F> vo;
#pragma unroll
        for (int ch = 0; ch < F; ++ch) vo.v[ch] = 0.f;
        if constexpr (BWD) vo = hg_load<F>(v_out + o);
        HgVec<F> res;
#pragma unroll
        for (int ch = 0; ch < F; ++ch) res.v[ch] = 0.f;
        if (!oob) {
            if (D == 3) {
                const float u3[3] = {u[0], u[1], u[2]};
                float g3[3] = {0.f, 0.f, 0.f};
                res = hg_level<3, F, STE, BWD>(lv, u3, vo, g3);
                if constexpr (BWD) {
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const uint32_t axis = (lv.dims >> (4 + 4 * d)) & 0xfu;
#pragma unroll
                        for (int k = 0; k < 3; ++k)
                            if (axis == (uint32_t)k) vp[k] += g3[d];
                    }
                }
            } else {
                const float u2[2] = {u[0], u[1]};
                float g2[2] = {0.f, 0.f};
                res = hg_level<2, F, STE, BWD>(lv, u2, vo, g2);
                if constexpr (BWD) {
#pragma unroll
                    for (int d = 0; d < 2; ++d) {
                        const uint32_t axis = (lv.dims >> (4 + 4 * d)) & 0xfu;
#pragma unroll
                        for (int k = 0; k < 3; ++k)
                            if (axis == (uint32_t)k) vp[k] += g2[d];
                    }
                }
            }
        }
        if constexpr (!BWD) hg_store<F>(out + o, res);
    }
    if constexpr (BWD) {
        if (v_pos != nullptr) { // (uniform) one owner per point sums its levels in level order: no atomics, same bits every run
            s_vu[tid * 3 + 0] = vp[0];
            s_vu[tid * 3 + 1] = vp[1];
            s_vu[tid * 3 + 2] = vp[2];
            __syncthreads();
            if (active && l == 0) {
                float sum[3] = {0.f, 0.f, 0.f};
                for (uint32_t j = 0; j < L; ++j) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) sum[k] += s_vu[(tid + j) * 3 + k];
                }
                for (uint32_t k = 0; k < a.pos_dim; ++k) v_pos[b * a.pos_dim + k] = sum[k];
            }
        }
    }
}

// validation + level table shared by both directions; returns 0 and fills `a`, or sets the error and returns 1
int32_t hashgrid_table(const char *fn, uint64_t n, uint32_t pos_dim, uint32_t n_grids, uint32_t F, const float *pos,
                       const float *const *params, float *const *v_params, const uint64_t *rows, const uint32_t *num_dim,
                       const uint32_t *axes, const uint32_t *n_levels, const int32_t *resolutions, const int32_t *offsets,
                       HgArgs &a) {
#define HG_CHECK(cond, msg)                       \
    do {                                          \
        if (!(cond)) {                            \
            gs_set_error("%s: %s", fn, msg);      \
            return 1;                             \
        }                                         \
    } while (0)
    HG_CHECK(pos && params && rows && num_dim && axes && n_levels && resolutions && offsets, "null pointer");
    HG_CHECK(pos_dim == 2 || pos_dim == 3, "pos_dim must be 2 or 3");
    HG_CHECK(n_grids >= 1 && n_grids <= HG_MAX_GRIDS, "n_grids must be in 1..4");
    HG_CHECK(F == 1 || F == 2 || F == 4, "n_features must be 1, 2 or 4");
    static const uint32_t axis_table[4][3] = {{0, 1, 2}, {0, 1, 0}, {0, 2, 0}, {1, 2, 0}};
    uint32_t total = 0;
    size_t cursor_r = 0, cursor_o = 0;
    for (uint32_t g = 0; g < n_grids; ++g) {
        HG_CHECK(params[g] != nullptr, "null pointer");
        HG_CHECK(((uintptr_t)params[g] % (4u * F)) == 0 && (!v_params || ((uintptr_t)v_params[g] % (4u * F)) == 0),
                 "tables must be aligned to n_features floats");
        HG_CHECK(num_dim[g] == 2 || num_dim[g] == 3, "num_dim must be 2 or 3");
        HG_CHECK(axes[g] <= 3 && (axes[g] == HG_AXES_XYZ) == (num_dim[g] == 3), "axes do not match num_dim");
        HG_CHECK(pos_dim == 3 || axes[g] == HG_AXES_XY, "axes outside the position's columns");
        HG_CHECK(n_levels[g] >= 1 && total + n_levels[g] <= HG_MAX_LEVELS, "1..32 levels in total");
        const int32_t *res = resolutions + cursor_r, *off = offsets + cursor_o;
        HG_CHECK(off[0] >= 0, "offsets must be ascending from >= 0");
        for (uint32_t l = 0; l < n_levels[g]; ++l) {
            HG_CHECK(res[l] >= 3 && (uint32_t)res[l] <= HG_MAX_RES, "resolution must be in 3..2^24");
            HG_CHECK(off[l + 1] > off[l], "offsets must be ascending (at least one row per level)");
        }
        HG_CHECK((uint64_t)off[n_levels[g]] <= rows[g], "offsets reach past the table");
        for (uint32_t l = 0; l < n_levels[g]; ++l) {
            HgLevel &lv = a.lv[total + l];
            lv.table = params[g] + (size_t)off[l] * F;
            lv.v_table = (v_params && v_params[g]) ? v_params[g] + (size_t)off[l] * F : nullptr;
            lv.T = (uint32_t)(off[l + 1] - off[l]);
            lv.R = (uint32_t)res[l];
            const uint32_t *ax = axis_table[axes[g]];
            lv.dims = num_dim[g] | ax[0] << 4 | ax[1] << 8 | ax[2] << 12;
            lv.pad_ = 0;
        }
        total += n_levels[g];
        cursor_r += n_levels[g];
        cursor_o += n_levels[g] + 1;
    }
    a.n = n;
    a.n_levels = total;
    a.pos_dim = pos_dim;
    a.ppb = 256u / total;
    a.pos = pos;
    HG_CHECK((n + a.ppb - 1) / a.ppb <= 0x7fffffffull, "too many points for one launch");
#undef HG_CHECK
    return 0;
}

template <bool BWD>
void hashgrid_launch(const HgArgs &a, uint32_t F, bool ste, float *out, const float *v_out, float *v_pos, hipStream_t st) {
    const dim3 grid((uint32_t)((a.n + a.ppb - 1) / a.ppb)), block(256);
#define HG_CASE(f)                                                                                          \
    if (F == f) {                                                                                           \
        if (ste)                                                                                            \
            hipLaunchKernelGGL((hashgrid_kernel<f, true, BWD>), grid, block, 0, st, a, out, v_out, v_pos);  \
        else                                                                                                \
            hipLaunchKernelGGL((hashgrid_kernel<f, false, BWD>), grid, block, 0, st, a, out, v_out, v_pos); \
    }
    HG_CASE(1) HG_CASE(2) HG_CASE(4)
#undef HG_CASE
}

// ---------------------------------------------------------------------------------------------------------------------
// Gaussian bits

constexpr float GB_SCALE_MIN = 1e-9f;
constexpr float GB_RSQRT2 = 0.70710678118654752f;
constexpr float GB_RSQRT2PI = 0.39894228040143268f;
constexpr float GB_LN2 = 0.69314718055994531f;

struct GbTerms {
    float a, b, s_inv, diff; // standardised bin edges (upper, lower), 1 / s, Phi(a) - Phi(b)
};

// Phi(a) - Phi(b) evaluated on the side where the complementary error functions are small: both tails keep their
// relative accuracy (0.5 (1 + erf) differences lose everything beyond ~5 sigma)
GS_DEV GbTerms gb_terms(float x, float hq, float mean, float scale_raw) {
    GbTerms t;
    const float s = fmaxf(scale_raw, GB_SCALE_MIN);
    t.s_inv = 1.f / s;
    const float d = x - mean;
    t.a = (d + hq) * t.s_inv;
    t.b = (d - hq) * t.s_inv;
    const float sg = (t.a + t.b) > 0.f ? 1.f : -1.f;
    t.diff = 0.5f * sg * (erfcf(sg * t.b * GB_RSQRT2) - erfcf(sg * t.a * GB_RSQRT2));
    return t;
}

template <bool BWD>
__global__ void __launch_bounds__(256) gaussian_bits_kernel(uint64_t total, uint32_t C, const float *__restrict__ x,
                                                             const float *__restrict__ net, const float *__restrict__ half_q,
                                                             float bound, float *__restrict__ bits,
                                                             const float *__restrict__ v_bits, float *__restrict__ v_x,
                                                             float *__restrict__ v_net) {
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t m = e / C;
        const uint32_t c = (uint32_t)(e - m * C);
        const size_t i_mean = (size_t)m * 2u * C + c, i_scale = i_mean + C;
        const float scale_raw = net[i_scale];
        const GbTerms t = gb_terms(x[e], half_q[c], net[i_mean], scale_raw);
        const float like = fabsf(t.diff);
        const float like_b = fmaxf(bound, like);
        if constexpr (!BWD) {
            bits[e] = -log2f(like_b);
        } else {
            const float g_like_b = -v_bits[e] / (GB_LN2 * like_b);
            const bool pass = (like >= bound) || (g_like_b < 0.f); // LowerBound
            const float sg = t.diff > 0.f ? 1.f : (t.diff < 0.f ? -1.f : 0.f);
            const float g_diff = pass ? g_like_b * sg : 0.f;
            const float g_a = g_diff * GB_RSQRT2PI * expf(-0.5f * t.a * t.a);
            const float g_b = -g_diff * GB_RSQRT2PI * expf(-0.5f * t.b * t.b);
            const float g_x = (g_a + g_b) * t.s_inv;
            const float g_s = -(g_a * t.a + g_b * t.b) * t.s_inv;
            v_x[e] = g_x;
            v_net[i_mean] = -g_x;
            v_net[i_scale] = scale_raw >= GB_SCALE_MIN ? g_s : 0.f; // clamp(min): passes where the raw scale is not below it
        }
    }
}

uint32_t gb_blocks(uint64_t total) {
    const uint64_t blocks = (total + 255) / 256;
    return (uint32_t)(blocks < (1u << 20) ? blocks : (1u << 20));
}

} // namespace

extern "C" int32_t gs_hashgrid_encode_fwd(uint64_t n, uint32_t pos_dim, uint32_t n_grids, uint32_t n_features,
                                          uint32_t ste_binary, const float *pos, const float *const *params,
                                          const uint64_t *rows, const uint32_t *num_dim, const uint32_t *axes,
                                          const uint32_t *n_levels, const int32_t *resolutions, const int32_t *offsets,
                                          float *out, gs_stream_t stream) {
    if (n == 0) return 0;
    HgArgs a;
    if (hashgrid_table(__func__, n, pos_dim, n_grids, n_features, pos, params, nullptr, rows, num_dim, axes, n_levels,
                       resolutions, offsets, a) != 0)
        return 1;
    GS_CHECK_ARG(out != nullptr, "null pointer");
    GS_CHECK_ARG(((uintptr_t)out % (4u * n_features)) == 0, "out must be aligned to n_features floats");
    hashgrid_launch<false>(a, n_features, ste_binary != 0, out, nullptr, nullptr, (hipStream_t)stream);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_hashgrid_encode_bwd(uint64_t n, uint32_t pos_dim, uint32_t n_grids, uint32_t n_features,
                                          uint32_t ste_binary, const float *pos, const float *const *params,
                                          const uint64_t *rows, const uint32_t *num_dim, const uint32_t *axes,
                                          const uint32_t *n_levels, const int32_t *resolutions, const int32_t *offsets,
                                          const float *v_out, float *const *v_params, float *v_pos, gs_stream_t stream) {
    if (n == 0) return 0;
    HgArgs a;
    if (hashgrid_table(__func__, n, pos_dim, n_grids, n_features, pos, params, v_params, rows, num_dim, axes, n_levels,
                       resolutions, offsets, a) != 0)
        return 1;
    GS_CHECK_ARG(v_out != nullptr, "null pointer");
    GS_CHECK_ARG(((uintptr_t)v_out % (4u * n_features)) == 0, "v_out must be aligned to n_features floats");
    hashgrid_launch<true>(a, n_features, ste_binary != 0, nullptr, v_out, v_pos, (hipStream_t)stream);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_gaussian_bits_fwd(uint64_t n_rows, uint32_t channels, const float *x, const float *net,
                                        const float *half_q, float likelihood_bound, float *bits, gs_stream_t stream) {
    if (n_rows == 0) return 0;
    GS_CHECK_ARG(channels >= 1 && channels <= 32, "channels must be in 1..32");
    GS_CHECK_ARG(x && net && half_q && bits, "null pointer");
    const uint64_t total = n_rows * channels;
    hipLaunchKernelGGL((gaussian_bits_kernel<false>), dim3(gb_blocks(total)), dim3(256), 0, (hipStream_t)stream, total,
                       channels, x, net, half_q, likelihood_bound, bits, nullptr, nullptr, nullptr);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_gaussian_bits_bwd(uint64_t n_rows, uint32_t channels, const float *x, const float *net,
                                        const float *half_q, float likelihood_bound, const float *v_bits, float *v_x,
                                        float *v_net, gs_stream_t stream) {
    if (n_rows == 0) return 0;
    GS_CHECK_ARG(channels >= 1 && channels <= 32, "channels must be in 1..32");
    GS_CHECK_ARG(x && net && half_q && v_bits && v_x && v_net, "null pointer");
    const uint64_t total = n_rows * channels;
    hipLaunchKernelGGL((gaussian_bits_kernel<true>), dim3(gb_blocks(total)), dim3(256), 0, (hipStream_t)stream, total,
                       channels, x, net, half_q, likelihood_bound, nullptr, v_bits, v_x, v_net);
    GS_CHECK_LAUNCH();
    return 0;
}
