// appearance.hip -- the static trainer's appearance module (--app_opt; reference examples/utils.py: AppearanceOptModule, called at
// examples/simple_trainer.py:766-774), forward and backward (gs_appearance_fwd / _bwd): per (camera c, splat n)
//   x   = cat(embed_c [E], features_n [F], bases(normalize(dir_cn)) [K], zero above the nb bases in use)
//   h1  = relu(W1 x + b1)   h2 = relu(W2 h1 + b2)   out = W3 h2 + b3 (+ base_n) (sigmoid when `activate`)
// with a hidden width of 64, on the matrix cores: __builtin_amdgcn_mfma_f32_32x32x2f32, exact f32 (an fmaf chain).
//
// Orientation.  Every product is H^T [unit x rows] = W [unit x in] . X^T [in x rows]: the weight is the A operand, the batch row
// sits on the lane (lane & 31; the two lane halves h = lane >> 5 split the k index) and the hidden unit in the accumulator
// registers: register r of tile t in lane half h is unit u(t, r, h) = 32 t + 8 (r >> 2) + (r & 3) + 4 h.  A layer's accumulator
// is therefore the next product's B operand as it stands -- register (t, r) is the k-step whose two k values are u(t, r, 0) and
// u(t, r, 1) -- and the weight (A) operand is read from LDS at that same permuted k.  Layer 1 takes its B operand from the wave's
// LDS image of the input rows (features staged coalesced, bases evaluated by the lane); layers 2 and 3 and the backward's data
// gradients (W^T . dZ, same shape) take theirs from registers.  Layer 3 (3 x 64) is VALU work: 96 fmas and one cross-half add.
// The embedding's share of layer 1, W1[:, :E] embed_c + b1, is constant per camera: 64 lanes compute it once per camera into LDS
// and it is the accumulator's initial value.
//
// Weight gradients sum over the batch row, which lives on the lanes, so their operands cross LDS transposed: a wave writes H1, H2,
// dZ2 and dZ1 as [unit][row] images (two buffers, reused) and reads them back with the unit on the lane; the running v_W1 and v_W2
// tiles stay in accumulator registers over every tile and camera a wave visits.  From the same images lane u sums its unit's 32
// rows for v_b2, v_W3 and d_pre (the gradient of the per-camera initial value: v_b1, v_W1[:, :E] and v_embeds follow from it by
// [C, 64] products that the caller does).  This is the LDS form for the weight-gradient operands and the register form for
// everything else.
//
// A workgroup keeps all weights in LDS for its lifetime; wave w of workgroup b owns the 32-row tiles b W + w, b W + w + G W, ... of
// n for EVERY camera (cameras are the outer loop), so v_features, v_means and v_base are summed over the cameras by the one lane
// that owns the row (plain load + add + store from the second camera on) and every wave's weight sums leave as one row of
// partials, added by the caller: no float atomics, bit-identical from run to run.
#include "gs_common.h"
#include "sh_bwd_lane.h"

#include <atomic>

#define AP_HID 64
#define AP_TS 36           // row stride of the transposed [unit][row] images: 16-byte aligned rows
#define AP_W2S 65          // row stride of W2 in LDS (odd: a column read over 32 units is conflict-free)
#define AP_MAX_BLOCKS 256      // backward: one workgroup per CU (its LDS allows no more)
#define AP_MAX_BLOCKS_FWD 512  // forward: two per CU
#define AP_LDS_BYTES (160 * 1024)

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

struct AppGeo {
    const float *features, *embeds, *dirs, *means, *cams;
    const float *w1, *b1, *w2, *b2, *w3, *b3, *base;
    uint32_t N, C, F, E, K, nb;
    int32_t deg, activate;
};

struct Row {
    float ux, uy, uz, inv, len;
    uint32_t n;
    bool valid;
};

GS_DEV constexpr int unit0(int t, int r) { return 32 * t + 8 * (r >> 2) + (r & 3); }  // unit u(t, r, h) = unit0(t, r) + 4 h
// (every LDS address below is one per-lane base plus a compile-time offset: addresses that depend on the lane half through an
// expression of their own are loop invariants that the compiler keeps in registers, hundreds of them)

// (LDS is in order within a wave: this only keeps the compiler from moving accesses across the hand-over between lanes)
GS_DEV void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// (keeps the scheduler from hoisting every operand load of an unrolled product in front of it: that spills)
GS_DEV void sched_fence() { __builtin_amdgcn_sched_barrier(0); }

GS_DEV f32x16 mfma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

template <int FT>
struct Lay {
    static constexpr int KX = 32 * FT + 32;  // in-kernel input columns: features (padded to 32 FT), then a tile of bases
    static constexpr int S1 = KX + 1;        // row stride of W1 and of the input image (odd)
    static constexpr int W1 = 0, W2 = W1 + AP_HID * S1, W3 = W2 + AP_HID * AP_W2S, B2 = W3 + 3 * AP_HID, B3 = B2 + AP_HID,
                         PRE = B3 + 4, WAVES = PRE + AP_HID;
    static constexpr int XS = 32 * S1;                                  // per wave, forward
    static constexpr int TA = XS, TB = TA + AP_HID * AP_TS, GS = TB + AP_HID * AP_TS, WAVE_BWD = GS + 96;  // per wave, backward
};

// weights -> LDS (W1 without its embedding columns, in the in-kernel column order, zero elsewhere); the waves' buffers are zeroed so
// that the padding columns of the input images stay zero for the whole kernel
template <int FT>
GS_DEV void load_weights(const AppGeo &g, float *smem, int total_floats) {
    typedef Lay<FT> L;
    for (int i = threadIdx.x; i < total_floats; i += blockDim.x) smem[i] = 0.f;
    __syncthreads();
    const int fk = g.F + g.K, D = g.E + fk;
    for (int i = threadIdx.x; i < AP_HID * fk; i += blockDim.x) {
        const int u = i / fk, col = i - u * fk;
        smem[L::W1 + u * L::S1 + (col < (int)g.F ? col : 32 * FT + col - (int)g.F)] = g.w1[u * D + g.E + col];
    }
    for (int i = threadIdx.x; i < AP_HID * AP_HID; i += blockDim.x) smem[L::W2 + (i >> 6) * AP_W2S + (i & 63)] = g.w2[i];
    for (int i = threadIdx.x; i < 3 * AP_HID; i += blockDim.x) smem[L::W3 + i] = g.w3[i];
    for (int i = threadIdx.x; i < AP_HID; i += blockDim.x) smem[L::B2 + i] = g.b2[i];
    if (threadIdx.x < 3) smem[L::B3 + threadIdx.x] = g.b3[threadIdx.x];
}

// the per-camera initial value of layer 1 (between two workgroup barriers: every wave has left the previous camera's tiles)
template <int FT>
GS_DEV void camera_pre(const AppGeo &g, float *smem, uint32_t c) {
    __syncthreads();
    if (threadIdx.x < AP_HID) {
        const int D = g.E + g.F + g.K;
        float p = g.b1[threadIdx.x];
        if (g.embeds)
            for (uint32_t e = 0; e < g.E; ++e) p = fmaf(g.w1[threadIdx.x * D + e], g.embeds[(size_t)c * g.E + e], p);
        smem[Lay<FT>::PRE + threadIdx.x] = p;
    }
    __syncthreads();
}

GS_DEV void eval_bases(int deg, float x, float y, float z, float *Y) {
#pragma unroll
    for (int k = 0; k < 32; ++k) Y[k] = 0.f;
    switch (deg) {
    case 0: sh_basis<0>(x, y, z, Y); break;
    case 1: sh_basis<1>(x, y, z, Y); break;
    case 2: sh_basis<2>(x, y, z, Y); break;
    case 3: sh_basis<3>(x, y, z, Y); break;
    default: sh_basis<4>(x, y, z, Y); break;
    }
}

// rows [32 tile, 32 tile + 32) of camera c -> the wave's input image xs[row][column]: features coalesced, the bases by the row's
// two lanes (half h writes bases 16 h .. 16 h + 15).  Rows past N are zero.
template <int FT>
GS_DEV void stage_tile(const AppGeo &g, uint32_t c, uint32_t tile, float *xs, int lane, Row &row) {
    typedef Lay<FT> L;
    const uint32_t n0 = tile * 32u, F = g.F;
    const uint32_t live = (g.N - n0 < 32u ? g.N - n0 : 32u) * F;
    const float *src = g.features + (size_t)n0 * F;
    for (uint32_t i = lane; i < 32u * F; i += GS_WAVE) {
        const uint32_t r = i / F, col = i - r * F;
        xs[r * L::S1 + col] = i < live ? src[i] : 0.f;
    }
    const int j = lane & 31, h = lane >> 5;
    row.n = n0 + j;
    row.valid = row.n < g.N;
    float dx = 0.f, dy = 0.f, dz = 0.f;
    if (row.valid) {
        if (g.dirs) {
            const float *d = g.dirs + ((size_t)c * g.N + row.n) * 3;
            dx = d[0], dy = d[1], dz = d[2];
        } else {
            const float *m = g.means + (size_t)row.n * 3, *o = g.cams + (size_t)c * 3;
            dx = m[0] - o[0], dy = m[1] - o[1], dz = m[2] - o[2];
        }
    }
    // F.normalize: x / max(||x||, 1e-12)
    row.len = sqrtf(dx * dx + dy * dy + dz * dz);
    row.inv = 1.f / fmaxf(row.len, 1e-12f);
    row.ux = dx * row.inv, row.uy = dy * row.inv, row.uz = dz * row.inv;
    float Y[32];
    eval_bases(g.deg, row.ux, row.uy, row.uz, Y);
    float *dst = xs + j * L::S1 + 32 * FT;
    if (h == 0) {
#pragma unroll
        for (int k = 0; k < 16; ++k) dst[k] = row.valid ? Y[k] : 0.f;
    } else {
#pragma unroll
        for (int k = 16; k < 32; ++k) dst[k] = row.valid ? Y[k] : 0.f;
    }
}

// H1^T = W1x . X^T from the initial value: k-step s of a segment holds columns 2 s (lane half 0) and 2 s + 1 (half 1)
template <int FT>
GS_DEV void layer1(const AppGeo &g, const float *smem, const float *xs, int lane, f32x16 acc[2]) {
    typedef Lay<FT> L;
    const int j = lane & 31, h = lane >> 5;
    const float *pre = smem + L::PRE + 4 * h;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const float4 p = *reinterpret_cast<const float4 *>(pre + 32 * t + 8 * q4);
            acc[t][4 * q4] = p.x, acc[t][4 * q4 + 1] = p.y, acc[t][4 * q4 + 2] = p.z, acc[t][4 * q4 + 3] = p.w;
        }
    const float *wa = smem + L::W1 + j * L::S1 + h, *wb = wa + 32 * L::S1, *xb = xs + j * L::S1 + h;
    const int fs = ((int)g.F + 1) >> 1, ks = ((int)g.nb + 1) >> 1;
    for (int s = 0; s < fs; ++s) {
        const float b = xb[2 * s];
        acc[0] = mfma(wa[2 * s], b, acc[0]);
        acc[1] = mfma(wb[2 * s], b, acc[1]);
    }
    for (int s = 16 * FT; s < 16 * FT + ks; ++s) {
        const float b = xb[2 * s];
        acc[0] = mfma(wa[2 * s], b, acc[0]);
        acc[1] = mfma(wb[2 * s], b, acc[1]);
    }
}

GS_DEV void relu2(f32x16 a[2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) a[t][r] = fmaxf(a[t][r], 0.f);
}

// out^T [64 x rows] = M . in^T, `in` in accumulator layout; M[u][k] at m[u * su + k * sk] (su, sk = AP_W2S, 1: W2; 1, AP_W2S: W2^T)
template <bool INIT_BIAS, int su, int sk>
GS_DEV void dense64(const float *m, const float *bias, int lane, const f32x16 in[2], f32x16 out[2]) {
    const int i = lane & 31, h = lane >> 5;
    const float *mb = m + i * su + 4 * h * sk, *bb = bias + 4 * h;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
            if (INIT_BIAS) p = *reinterpret_cast<const float4 *>(bb + 32 * t + 8 * q4);
            out[t][4 * q4] = p.x, out[t][4 * q4 + 1] = p.y, out[t][4 * q4 + 2] = p.z, out[t][4 * q4 + 3] = p.w;
        }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float b = in[t][r];
            out[0] = mfma(mb[unit0(t, r) * sk], b, out[0]);
            out[1] = mfma(mb[32 * su + unit0(t, r) * sk], b, out[1]);
            if ((r & 3) == 3) sched_fence();
        }
}

// s[c] = W3[c] . h2 + b3[c] (+ base): each lane half sums its 32 units, the halves are added (the same value in both)
GS_DEV void layer3(const AppGeo &g, const float *w3s, const float *b3s, int lane, const f32x16 h2[2], const Row &row, float s[3]) {
    const float *wl = w3s + 4 * (lane >> 5);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float p = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const float4 w = *reinterpret_cast<const float4 *>(wl + c * AP_HID + 32 * t + 8 * q4);
                p = fmaf(w.x, h2[t][4 * q4], p);
                p = fmaf(w.y, h2[t][4 * q4 + 1], p);
                p = fmaf(w.z, h2[t][4 * q4 + 2], p);
                p = fmaf(w.w, h2[t][4 * q4 + 3], p);
            }
        p += __shfl_xor(p, 32);
        p += b3s[c];
        if (g.base && row.valid) p += g.base[(size_t)row.n * 3 + c];
        s[c] = p;
    }
}

GS_DEV float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

template <int FT>
__global__ void __launch_bounds__(GS_BLOCK) appearance_fwd_kernel(AppGeo g, float *__restrict__ out, int lds_floats) {
    typedef Lay<FT> L;
    extern __shared__ __align__(16) float ap_lds[];
    const int nw = blockDim.x >> 6, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *xs = ap_lds + L::WAVES + w * L::XS;
    load_weights<FT>(g, ap_lds, lds_floats);
    const uint32_t tiles = (g.N + 31u) >> 5, step = gridDim.x * nw;
    for (uint32_t c = 0; c < g.C; ++c) {
        camera_pre<FT>(g, ap_lds, c);
        for (uint32_t tile = blockIdx.x * nw + w; tile < tiles; tile += step) {
            Row row;
            stage_tile<FT>(g, c, tile, xs, lane, row);
            wave_sync();
            f32x16 h1[2], h2[2];
            layer1<FT>(g, ap_lds, xs, lane, h1);
            wave_sync();  // (the next tile overwrites xs)
            relu2(h1);
            dense64<true, AP_W2S, 1>(ap_lds + L::W2, ap_lds + L::B2, lane, h1, h2);
            relu2(h2);
            float s[3];
            layer3(g, ap_lds + L::W3, ap_lds + L::B3, lane, h2, row, s);
            if (row.valid && lane < 32) {
                float *o = out + ((size_t)c * g.N + row.n) * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) o[k] = g.activate ? sigmoidf(s[k]) : s[k];
            }
        }
    }
}

// accumulator layout -> the [unit][row] image
GS_DEV void store_transposed(float *T, int lane, const f32x16 a[2]) {
    float *tb = T + 4 * (lane >> 5) * AP_TS + (lane & 31);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) tb[unit0(t, r) * AP_TS] = a[t][r];
}

GS_DEV float row_sum(const float *T, int lane, float acc) {
    const float *tl = T + lane * AP_TS;
#pragma unroll 1
    for (int u = 0; u < 8; ++u) {
        const float4 v = *reinterpret_cast<const float4 *>(tl + 4 * u);
        acc += v.x, acc += v.y, acc += v.z, acc += v.w;
    }
    return acc;
}

struct BwdOut {
    float *v_features, *v_dirs, *v_means, *v_base, *partials;
};

GS_DEV void basis_grad(int deg, float x, float y, float z, const float *w, float &gx, float &gy, float &gz) {
    switch (deg) {
    case 0: gx = gy = gz = 0.f; break;
    case 1: sh_basis_grad_contract<1>(x, y, z, w, gx, gy, gz); break;
    case 2: sh_basis_grad_contract<2>(x, y, z, w, gx, gy, gz); break;
    case 3: sh_basis_grad_contract<3>(x, y, z, w, gx, gy, gz); break;
    default: sh_basis_grad_contract<4>(x, y, z, w, gx, gy, gz); break;
    }
}

// A wave's row of partials: v_W1 without the embedding columns [64, F + K], v_W2 [64, 64], v_W3 [3, 64], v_b2 [64], v_b3 [3], one
// float of padding, d_pre [C, 64].
template <int FT>
__global__ void __launch_bounds__(GS_BLOCK) appearance_bwd_kernel(AppGeo g, const float *__restrict__ v_out, BwdOut o, int lds_floats) {
    typedef Lay<FT> L;
    extern __shared__ __align__(16) float ap_lds[];
    const int nw = blockDim.x >> 6, w = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    float *xs = ap_lds + L::WAVES + w * L::WAVE_BWD, *TA = xs + L::TA, *TB = xs + L::TB, *gs = xs + L::GS;
    load_weights<FT>(g, ap_lds, lds_floats);
    const float *w1s = ap_lds + L::W1, *w2s = ap_lds + L::W2, *w3s = ap_lds + L::W3;
    const float *w3l = w3s + 4 * h, *w1l = w1s + 4 * h * L::S1 + j, *xl = xs + 16 * h * L::S1 + j;
    const float *tbu = TB + lane * AP_TS;                                        // lane = unit
    const float *tar = TA + j * AP_TS + 16 * h, *tbr = TB + j * AP_TS + 16 * h;  // lane = unit of a 32-unit tile, k = rows
    const uint32_t tiles = (g.N + 31u) >> 5, step = gridDim.x * nw;
    const int fk = g.F + g.K;
    const size_t row_len = (size_t)AP_HID * fk + AP_HID * AP_HID + 3 * AP_HID + AP_HID + 4 + (size_t)g.C * AP_HID;
    float *part = o.partials + ((size_t)blockIdx.x * nw + w) * row_len;
    float *part_w2 = part + (size_t)AP_HID * fk, *part_w3 = part_w2 + AP_HID * AP_HID, *part_b2 = part_w3 + 3 * AP_HID,
          *part_b3 = part_b2 + AP_HID, *part_pre = part_b3 + 4;

    f32x16 dW1[2][FT + 1], dW2[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int b = 0; b < FT + 1; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) dW1[a][b][r] = 0.f;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) dW2[a][b][r] = 0.f;
    }
    float dw3[3] = {0.f, 0.f, 0.f}, db2 = 0.f, db3 = 0.f;

    for (uint32_t c = 0; c < g.C; ++c) {
        camera_pre<FT>(g, ap_lds, c);
        float dpre = 0.f;
        for (uint32_t tile = blockIdx.x * nw + w; tile < tiles; tile += step) {
            Row row;
            stage_tile<FT>(g, c, tile, xs, lane, row);
            wave_sync();
            // -- forward, recomputed; H1 and H2 leave their [unit][row] images
            f32x16 h1[2], h2[2];
            layer1<FT>(g, ap_lds, xs, lane, h1);
            relu2(h1);
            store_transposed(TA, lane, h1);
            uint32_t alive1 = 0, alive2 = 0;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) alive1 |= (h1[t][r] > 0.f ? 1u : 0u) << (16 * t + r);
            dense64<true, AP_W2S, 1>(w2s, ap_lds + L::B2, lane, h1, h2);
            relu2(h2);
            store_transposed(TB, lane, h2);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) alive2 |= (h2[t][r] > 0.f ? 1u : 0u) << (16 * t + r);
            float s[3], gr[3];
            layer3(g, w3s, ap_lds + L::B3, lane, h2, row, s);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                gr[k] = 0.f;
                if (row.valid) {
                    gr[k] = v_out[((size_t)c * g.N + row.n) * 3 + k];
                    if (g.activate) {
                        const float sg = sigmoidf(s[k]);
                        gr[k] *= sg * (1.f - sg);
                    }
                }
                if (h == 0) gs[k * 32 + j] = gr[k];
            }
            if (o.v_base && row.valid && h == 0) {
                float *vb = o.v_base + (size_t)row.n * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) vb[k] = c ? vb[k] + gr[k] : gr[k];
            }
            // -- dZ2 = (h2 > 0) W3^T g, in accumulator layout
            f32x16 dz2[2];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const int u0 = 32 * t + 8 * q4;
                    const float4 wa = *reinterpret_cast<const float4 *>(w3l + u0), wb = *reinterpret_cast<const float4 *>(w3l + AP_HID + u0),
                                 wc = *reinterpret_cast<const float4 *>(w3l + 2 * AP_HID + u0);
                    const float a4[4] = {wa.x, wa.y, wa.z, wa.w}, b4[4] = {wb.x, wb.y, wb.z, wb.w}, c4[4] = {wc.x, wc.y, wc.z, wc.w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float v = fmaf(c4[q], gr[2], fmaf(b4[q], gr[1], a4[q] * gr[0]));
                        dz2[t][4 * q4 + q] = ((alive2 >> (16 * t + 4 * q4 + q)) & 1u) ? v : 0.f;
                    }
                }
            wave_sync();
            // -- lane = unit: v_W3 and v_b3 from the H2 image and g (rolled: unrolled, all 32 loads are issued first and spill)
#pragma unroll 1
            for (int u = 0; u < 8; ++u) {
                const float4 hv = *reinterpret_cast<const float4 *>(tbu + 4 * u);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float4 gv = *reinterpret_cast<const float4 *>(gs + k * 32 + 4 * u);
                    dw3[k] = fmaf(gv.w, hv.w, fmaf(gv.z, hv.z, fmaf(gv.y, hv.y, fmaf(gv.x, hv.x, dw3[k]))));
                }
            }
            if (lane < 3) {
#pragma unroll 1
                for (int u = 0; u < 8; ++u) {
                    const float4 gv = *reinterpret_cast<const float4 *>(gs + lane * 32 + 4 * u);
                    db3 += gv.x, db3 += gv.y, db3 += gv.z, db3 += gv.w;
                }
            }
            wave_sync();
            store_transposed(TB, lane, dz2);
            wave_sync();
            db2 = row_sum(TB, lane, db2);
            // -- v_W2 [u2][u1] += dZ2 [u2 x rows] . H1^T [rows x u1]: k-step s holds rows s (lane half 0) and 16 + s (half 1)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float4 a[2], b[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    a[t] = *reinterpret_cast<const float4 *>(tbr + 32 * t * AP_TS + 4 * u);
                    b[t] = *reinterpret_cast<const float4 *>(tar + 32 * t * AP_TS + 4 * u);
                }
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
                    for (int t1 = 0; t1 < 2; ++t1) {
                        dW2[t2][t1] = mfma(a[t2].x, b[t1].x, dW2[t2][t1]);
                        dW2[t2][t1] = mfma(a[t2].y, b[t1].y, dW2[t2][t1]);
                        dW2[t2][t1] = mfma(a[t2].z, b[t1].z, dW2[t2][t1]);
                        dW2[t2][t1] = mfma(a[t2].w, b[t1].w, dW2[t2][t1]);
                    }
                sched_fence();
            }
            // -- dZ1 = (h1 > 0) W2^T dZ2
            f32x16 dz1[2];
            dense64<false, 1, AP_W2S>(w2s, w2s, lane, dz2, dz1);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) dz1[t][r] = ((alive1 >> (16 * t + r)) & 1u) ? dz1[t][r] : 0.f;
            wave_sync();
            store_transposed(TA, lane, dz1);
            wave_sync();
            dpre = row_sum(TA, lane, dpre);
            // -- v_W1 [u1][column] += dZ1 [u1 x rows] . X [rows x columns]
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float4 a[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) a[t] = *reinterpret_cast<const float4 *>(tar + 32 * t * AP_TS + 4 * u);
#pragma unroll
                for (int mt = 0; mt < FT + 1; ++mt) {
                    const float *xb = xl + 4 * u * L::S1 + 32 * mt;
                    const float b0 = xb[0], b1 = xb[L::S1], b2 = xb[2 * L::S1], b3 = xb[3 * L::S1];
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        dW1[t][mt] = mfma(a[t].x, b0, dW1[t][mt]);
                        dW1[t][mt] = mfma(a[t].y, b1, dW1[t][mt]);
                        dW1[t][mt] = mfma(a[t].z, b2, dW1[t][mt]);
                        dW1[t][mt] = mfma(a[t].w, b3, dW1[t][mt]);
                    }
                    sched_fence();
                }
            }
            wave_sync();  // (the feature tiles of dX overwrite the input image that the v_W1 products read across lanes)
            // -- dX = W1x^T dZ1, a tile of 32 input columns at a time: the feature tiles are stored, the bases' goes on to the direction
#pragma unroll
            for (int mt = 0; mt < FT + 1; ++mt) {
                if (mt < FT ? o.v_features == nullptr : (g.deg < 1 || (o.v_dirs == nullptr && o.v_means == nullptr))) continue;
                f32x16 dx;
#pragma unroll
                for (int r = 0; r < 16; ++r) dx[r] = 0.f;
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        dx = mfma(w1l[unit0(t, r) * L::S1 + 32 * mt], dz1[t][r], dx);
                        if ((r & 3) == 3) sched_fence();
                    }
                if (mt < FT) {
                    // (through the input image, which nothing reads any more: its padding columns get W1x's zero columns' exact zeros)
                    float *xd = xs + j * L::S1 + 4 * h + 32 * mt;
#pragma unroll
                    for (int r = 0; r < 16; ++r) xd[unit0(0, r)] = dx[r];
                } else {
                    // this lane half's bases in use: basis k sits in register 4 (k >> 3) + (k & 3) of half (k >> 2) & 1
                    float wy[25];
#pragma unroll
                    for (int k = 0; k < 25; ++k)
                        wy[k] = (((k >> 2) & 1) == h && k < (int)g.nb) ? dx[4 * (k >> 3) + (k & 3)] : 0.f;
                    float gx, gy, gz;
                    basis_grad(g.deg, row.ux, row.uy, row.uz, wy, gx, gy, gz);
                    gx += __shfl_xor(gx, 32), gy += __shfl_xor(gy, 32), gz += __shfl_xor(gz, 32);
                    // through x / max(||x||, 1e-12)
                    if (row.len > 1e-12f) {
                        const float d = gx * row.ux + gy * row.uy + gz * row.uz;
                        gx -= d * row.ux, gy -= d * row.uy, gz -= d * row.uz;
                    }
                    gx *= row.inv, gy *= row.inv, gz *= row.inv;
                    if (row.valid && h == 0) {
                        if (o.v_dirs) {
                            float *vd = o.v_dirs + ((size_t)c * g.N + row.n) * 3;
                            vd[0] = gx, vd[1] = gy, vd[2] = gz;
                        } else {
                            float *vm = o.v_means + (size_t)row.n * 3;
                            vm[0] = c ? vm[0] + gx : gx, vm[1] = c ? vm[1] + gy : gy, vm[2] = c ? vm[2] + gz : gz;
                        }
                    }
                }
            }
            if (o.v_features) {
                wave_sync();
                const uint32_t n0 = tile * 32u, F = g.F, live = (g.N - n0 < 32u ? g.N - n0 : 32u) * F;
                float *dst = o.v_features + (size_t)n0 * F;
                for (uint32_t i = lane; i < live; i += GS_WAVE) {
                    const uint32_t r = i / F, col = i - r * F;
                    const float v = xs[r * L::S1 + col];
                    dst[i] = c ? dst[i] + v : v;
                }
            }
            wave_sync();  // (the next tile overwrites the images)
        }
        part_pre[(size_t)c * AP_HID + lane] = dpre;
    }
    // -- the wave's sums
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int u = unit0(t, r) + 4 * h;
#pragma unroll
            for (int mt = 0; mt < FT + 1; ++mt) {
                const int col = 32 * mt + j;
                if (mt < FT) {
                    if (col < (int)g.F) part[(size_t)u * fk + col] = dW1[t][mt][r];
                } else if (j < (int)g.K) {
                    part[(size_t)u * fk + g.F + j] = dW1[t][mt][r];
                }
            }
#pragma unroll
            for (int t1 = 0; t1 < 2; ++t1) part_w2[u * AP_HID + 32 * t1 + j] = dW2[t][t1][r];
        }
#pragma unroll
    for (int k = 0; k < 3; ++k) part_w3[k * AP_HID + lane] = dw3[k];
    part_b2[lane] = db2;
    if (lane < 4) part_b3[lane] = lane < 3 ? db3 : 0.f;
}

struct AppPlan {
    int ft, waves_fwd, waves_bwd;
    size_t lds_fwd, lds_bwd;
};

template <int FT>
void plan_ft(AppPlan &p) {
    typedef Lay<FT> L;
    p.ft = FT;
    p.waves_fwd = p.waves_bwd = 0;
    for (int w = 4; w >= 1 && !p.waves_fwd; --w)
        if ((size_t)(L::WAVES + w * L::XS) * 4 <= AP_LDS_BYTES) p.waves_fwd = w;
    for (int w = 4; w >= 1 && !p.waves_bwd; --w)
        if ((size_t)(L::WAVES + w * L::WAVE_BWD) * 4 <= AP_LDS_BYTES) p.waves_bwd = w;
    p.lds_fwd = (size_t)(L::WAVES + p.waves_fwd * L::XS) * 4;
    p.lds_bwd = (size_t)(L::WAVES + p.waves_bwd * L::WAVE_BWD) * 4;
}

int32_t app_plan(const char *fn, uint32_t F, uint32_t E, uint32_t K, AppPlan &p) {
    // (F <= 96: with a fourth feature tile the backward's running v_W1 tiles no longer fit the register file without scratch)
    if (F == 0 || F > 96 || K == 0 || K > 25 || (uint64_t)E + F + K > 128) {
        gs_set_error("%s: unsupported sizes F = %u, E = %u, K = %u (1 <= F <= 96, 1 <= K <= 25, E + F + K <= 128)", fn, F, E, K);
        return 1;
    }
    switch ((F + 31) / 32) {
    case 1: plan_ft<1>(p); break;
    case 2: plan_ft<2>(p); break;
    default: plan_ft<3>(p); break;
    }
    return 0;
}

uint32_t app_blocks(uint32_t N, int waves, uint32_t max_blocks, uint32_t dflt = AP_MAX_BLOCKS) {
    const uint32_t cap = max_blocks && max_blocks < dflt ? max_blocks : dflt;  // a cap: never above the default
    const uint32_t need = gs_div_up(gs_div_up(N, 32), waves);
    return need < cap ? (need ? need : 1) : cap;
}

int32_t app_geo(const char *fn, AppGeo &g, uint32_t N, uint32_t C, uint32_t F, uint32_t E, uint32_t K, uint32_t nb, const float *features,
                const float *embeds, const float *dirs, const float *means, const float *cam_centers, const float *w1, const float *b1,
                const float *w2, const float *b2, const float *w3, const float *b3, const float *base, int32_t activate) {
    if (!features || !w1 || !b1 || !w2 || !b2 || !w3 || !b3) {
        gs_set_error("%s: null pointer (features and the six weight / bias arrays are required)", fn);
        return 1;
    }
    if (!dirs && !(means && cam_centers)) {
        gs_set_error("%s: null pointer (either dirs, or means and cam_centers)", fn);
        return 1;
    }
    if (N == 0 || C == 0 || N > 0x7fffffe0u) {
        gs_set_error("%s: unsupported shape N = %u, C = %u", fn, N, C);
        return 1;
    }
    int deg = -1;
    for (int d = 0; d <= 4; ++d)
        if (nb == (uint32_t)((d + 1) * (d + 1))) deg = d;
    if (deg < 0 || nb > K) {
        gs_set_error("%s: %u bases in use (a square, at most K = %u)", fn, nb, K);
        return 1;
    }
    const uintptr_t all = (uintptr_t)features | (uintptr_t)embeds | (uintptr_t)dirs | (uintptr_t)means | (uintptr_t)cam_centers |
                          (uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)w2 | (uintptr_t)b2 | (uintptr_t)w3 | (uintptr_t)b3 | (uintptr_t)base;
    if (all % 4 != 0) {
        gs_set_error("%s: misaligned pointer (floats need 4-byte alignment)", fn);
        return 1;
    }
    g.features = features, g.embeds = E ? embeds : nullptr, g.dirs = dirs, g.means = means, g.cams = cam_centers;
    g.w1 = w1, g.b1 = b1, g.w2 = w2, g.b2 = b2, g.w3 = w3, g.b3 = b3, g.base = base;
    g.N = N, g.C = C, g.F = F, g.E = E, g.K = K, g.nb = nb;
    g.deg = deg, g.activate = activate;
    return 0;
}

// more than 64 KB of dynamic LDS needs the attribute once per kernel and device: `slot` names the kernel (its size is fixed), a bit
// per device remembers that it is set
template <typename Kern>
int32_t app_lds(const char *fn, Kern kern, size_t bytes, int slot) {
    static std::atomic<uint64_t> done[8];
    if (bytes <= 64 * 1024) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 64;
    const uint64_t bit = dev >= 0 && dev < 64 ? 1ull << dev : 0;
    if (done[slot].load(std::memory_order_relaxed) & bit) return 0;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
        gs_set_error("%s: cannot reserve %zu bytes of LDS: %s", fn, bytes, hipGetErrorString(e));
        return 2;
    }
    done[slot].fetch_or(bit, std::memory_order_relaxed);
    return 0;
}

}  // namespace

extern "C" uint32_t gs_appearance_partial_rows(uint32_t N, uint32_t F, uint32_t E, uint32_t K, uint32_t max_blocks) {
    AppPlan p;
    if (app_plan("gs_appearance_partial_rows", F, E, K, p)) return 0;
    return app_blocks(N, p.waves_bwd, max_blocks) * p.waves_bwd;
}

extern "C" uint64_t gs_appearance_partial_cols(uint32_t C, uint32_t F, uint32_t K) {
    return (uint64_t)AP_HID * (F + K) + AP_HID * AP_HID + 3 * AP_HID + AP_HID + 4 + (uint64_t)C * AP_HID;
}

extern "C" int32_t gs_appearance_fwd(uint32_t N, uint32_t C, uint32_t F, uint32_t E, uint32_t K, uint32_t num_bases,
                                     const float *features, const float *embeds, const float *dirs, const float *means,
                                     const float *cam_centers, const float *w1, const float *b1, const float *w2, const float *b2,
                                     const float *w3, const float *b3, const float *base, int32_t activate, uint32_t max_blocks,
                                     float *colors, gs_stream_t stream) {
    const char *fn = "gs_appearance_fwd";
    AppPlan p;
    AppGeo g;
    if (app_plan(fn, F, E, K, p)) return 1;
    if (app_geo(fn, g, N, C, F, E, K, num_bases, features, embeds, dirs, means, cam_centers, w1, b1, w2, b2, w3, b3, base, activate))
        return 1;
    GS_CHECK_ARG(colors, "null pointer: no output");
    GS_CHECK_ARG((uintptr_t)colors % 4 == 0, "colors must be 4-byte aligned");
    const dim3 grid(app_blocks(N, p.waves_fwd, max_blocks, AP_MAX_BLOCKS_FWD)), block(p.waves_fwd * GS_WAVE);
    const hipStream_t st = (hipStream_t)stream;
    const int lf = (int)(p.lds_fwd / 4);
#define AP_FWD(FT_)                                                                                   \
    do {                                                                                              \
        if (int32_t r_ = app_lds(fn, appearance_fwd_kernel<FT_>, p.lds_fwd, FT_ - 1)) return r_;               \
        hipLaunchKernelGGL(appearance_fwd_kernel<FT_>, grid, block, p.lds_fwd, st, g, colors, lf);    \
    } while (0)
    switch (p.ft) {
    case 1: AP_FWD(1); break;
    case 2: AP_FWD(2); break;
    default: AP_FWD(3); break;
    }
#undef AP_FWD
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_appearance_bwd(uint32_t N, uint32_t C, uint32_t F, uint32_t E, uint32_t K, uint32_t num_bases,
                                     const float *features, const float *embeds, const float *dirs, const float *means,
                                     const float *cam_centers, const float *w1, const float *b1, const float *w2, const float *b2,
                                     const float *w3, const float *b3, const float *base, int32_t activate, const float *v_colors,
                                     uint32_t max_blocks, float *v_features, float *v_dirs, float *v_means, float *v_base,
                                     float *partials, gs_stream_t stream) {
    const char *fn = "gs_appearance_bwd";
    AppPlan p;
    AppGeo g;
    if (app_plan(fn, F, E, K, p)) return 1;
    if (app_geo(fn, g, N, C, F, E, K, num_bases, features, embeds, dirs, means, cam_centers, w1, b1, w2, b2, w3, b3, base, activate))
        return 1;
    GS_CHECK_ARG(v_colors, "null pointer: no upstream gradient");
    GS_CHECK_ARG(partials, "null pointer: no partials");
    GS_CHECK_ARG(!(v_dirs && v_means), "v_dirs and v_means are alternatives");
    GS_CHECK_ARG(!(v_dirs && !dirs) && !(v_means && dirs), "v_dirs goes with dirs, v_means with means and cam_centers");
    GS_CHECK_ARG(((uintptr_t)v_colors | (uintptr_t)v_features | (uintptr_t)v_dirs | (uintptr_t)v_means | (uintptr_t)v_base |
                  (uintptr_t)partials) % 4 == 0, "the gradient arrays must be 4-byte aligned");
    BwdOut o{v_features, v_dirs, v_means, v_base, partials};
    const dim3 grid(app_blocks(N, p.waves_bwd, max_blocks)), block(p.waves_bwd * GS_WAVE);
    const hipStream_t st = (hipStream_t)stream;
    const int lf = (int)(p.lds_bwd / 4);
#define AP_BWD(FT_)                                                                                      \
    do {                                                                                                 \
        if (int32_t r_ = app_lds(fn, appearance_bwd_kernel<FT_>, p.lds_bwd, 3 + FT_ - 1)) return r_;                  \
        hipLaunchKernelGGL(appearance_bwd_kernel<FT_>, grid, block, p.lds_bwd, st, g, v_colors, o, lf);  \
    } while (0)
    switch (p.ft) {
    case 1: AP_BWD(1); break;
    case 2: AP_BWD(2); break;
    default: AP_BWD(3); break;
    }
#undef AP_BWD
    GS_CHECK_LAUNCH();
    return 0;
}
