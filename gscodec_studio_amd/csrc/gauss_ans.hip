// gauss_ans.hip -- the hash-grid Gaussian route of the on-disk entropy coder: byte-wise rANS over many independent streams in
// which EVERY SYMBOL HAS ITS OWN FREQUENCIES, predicted from the splat's position (gfx950).
//
// The reference's _compress_gaussian_ans / _decompress_gaussian_ans (gsplat/compression/entropy_coding_compression.py:491-654) hand
// float64 means and standard deviations to constriction's QuantizedGaussian and rely on encoder and decoder regenerating
// bit-identical float32 MLP outputs from cuBLAS.  Here the bitstream is the library's own: its definition is the numpy module
// gscodec_studio_amd/compression/gauss_ans_reference.py, and every kernel below writes what that module writes.
//
//   model of a symbol: mu_q (mean on a grid of 8 steps per symbol, 0..2040), k (scale level 0..63), one table G uint16 [64, 4073]
//   cum(0) = 0, cum(256) = 2^16, cum(s) = G[k][8 s - 4 - mu_q + 2036] + s;  f(s) = cum(s + 1) - cum(s) >= 1 for every s
//
// gauss_ans_params_kernel: one lane per splat runs the regressor's MLP (Linear(48, 5C), ReLU, Linear(5C, 2C)) on the features the
// hash-grid encoder wrote, in the one float32 order regress_params states (accumulator starts at the bias, inputs ascending, every
// product and sum rounded on its own: this file is compiled with -ffp-contract=off and the functions carry GS_FP_STRICT), then the
// two normalisations and the quantisation to (mu_q, k).  The weights are wave-uniform LDS reads (broadcasts).  A splat's model thus
// depends on its features, the stored weights and mins / maxs alone -- not on a GEMM library's algorithm choice, N or the launch shape.
//
// Encoder and decoder are ans_stream_dev.h's streams at P = 16 under this model; G (521 KB) is read from global memory and lives
// in L2.  A lane emits at most 2 S + S / 512 bytes (a symbol costs at most 16 + log2(1 + 2^-7) bits: gauss_ans_reference.py derives
// it); the slot is that + 8.  The decoder's 8-step binary search on cum has a fixed trip count: nothing to spin on in a damaged stream.
#include "ans_stream_dev.h"

namespace {

constexpr uint32_t GA_P = 16, GA_K = 64, GA_WIDTH = 4073;
constexpr int32_t GA_MU_MAX = 2040, GA_T_MAX = 2036;
constexpr uint32_t GA_MAX_C = 8; // of the params kernel (weights in LDS, accumulators in registers)
constexpr uint32_t GA_MAX_C_CODER = 16;
constexpr uint32_t GA_IN = 48, GA_HID_PER_C = 5;
constexpr float GA_SCALE_MIN = 1e-9f;
constexpr uint32_t GA_STATUS_MODEL = 1u;

__host__ __device__ inline uint32_t ga_slot_bytes(uint32_t S) { return 2u * S + S / 512u + 8u; }

// cum(s) for s in 1..255 (mu_q, k already clamped into range): the index is clamped too, whatever the inputs
GS_DEV uint32_t ga_cum_mid(const uint16_t *__restrict__ G, uint32_t k, int32_t mu_q, uint32_t s) {
    int32_t t = 8 * (int32_t)s - 4 - mu_q;
    t = t < -GA_T_MAX ? -GA_T_MAX : (t > GA_T_MAX ? GA_T_MAX : t);
    return (uint32_t)G[k * GA_WIDTH + (uint32_t)(t + GA_T_MAX)] + s;
}

GS_DEV uint32_t ga_cum(const uint16_t *__restrict__ G, uint32_t k, int32_t mu_q, uint32_t s) {
    if (s == 0u) return 0u;
    if (s >= 256u) return 1u << GA_P;
    return ga_cum_mid(G, k, mu_q, s);
}

template <int C>
__global__ void __launch_bounds__(GS_BLOCK) gauss_ans_params_kernel(uint64_t N, const float *__restrict__ feat, const float *__restrict__ w1,
                                                                    const float *__restrict__ b1, const float *__restrict__ w2,
                                                                    const float *__restrict__ b2, const float *__restrict__ mins,
                                                                    const float *__restrict__ maxs, const float *__restrict__ tau,
                                                                    int16_t *__restrict__ mu_q, uint8_t *__restrict__ k_out,
                                                                    float *__restrict__ miu_out, float *__restrict__ sigma_out) {
    GS_FP_STRICT;
    constexpr int H = GA_HID_PER_C * C;
    __shared__ float s_w1[H * GA_IN]; // [j][i], as nn.Linear stores it
    __shared__ float s_b1[H];
    __shared__ float s_w2[2 * C * H];
    __shared__ float s_b2[2 * C];
    __shared__ float s_tau[GA_K - 1];
    for (uint32_t j = threadIdx.x; j < (uint32_t)(H * GA_IN); j += GS_BLOCK) s_w1[j] = w1[j];
    for (uint32_t j = threadIdx.x; j < (uint32_t)(2 * C * H); j += GS_BLOCK) s_w2[j] = w2[j];
    if (threadIdx.x < (uint32_t)H) s_b1[threadIdx.x] = b1[threadIdx.x];
    if (threadIdx.x < (uint32_t)(2 * C)) s_b2[threadIdx.x] = b2[threadIdx.x];
    if (threadIdx.x < GA_K - 1) s_tau[threadIdx.x] = tau[threadIdx.x];
    __syncthreads();
    const uint64_t n = (uint64_t)blockIdx.x * GS_BLOCK + threadIdx.x;
    if (n >= N) return;
    float h[H];
#pragma unroll
    for (int j = 0; j < H; ++j) h[j] = s_b1[j];
    const float4 *row = reinterpret_cast<const float4 *>(feat + n * GA_IN); // rows of 192 bytes: 16-byte aligned
#pragma unroll
    for (int q = 0; q < (int)GA_IN / 4; ++q) {
        const float4 v = row[q];
        const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int j = 0; j < H; ++j) {
                const float p = x[e] * s_w1[j * GA_IN + q * 4 + e];
                h[j] = h[j] + p;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < H; ++j) h[j] = h[j] > 0.f ? h[j] : 0.f;
    float o[2 * C];
#pragma unroll
    for (int m = 0; m < 2 * C; ++m) {
        float acc = s_b2[m];
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const float p = h[j] * s_w2[m * H + j];
            acc = acc + p;
        }
        o[m] = acc;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float miu = o[c];
        const float sigma = o[C + c] < GA_SCALE_MIN ? GA_SCALE_MIN : o[C + c];
        const float lo = mins[c];
        const float d = maxs[c] - lo;
        const float mu_norm = __fdiv_rn(miu - lo, d) * 255.f;
        const float sigma_norm = __fdiv_rn(sigma, d) * 255.f;
        int32_t mq = 0;
        if (mu_norm >= 255.f) mq = GA_MU_MAX;
        else if (mu_norm > 0.f) mq = (int32_t)rintf(mu_norm * 8.f);
        uint32_t kk = 0u;
        for (uint32_t j = 0; j < GA_K - 1; ++j) kk += s_tau[j] <= sigma_norm ? 1u : 0u;
        mu_q[(uint64_t)c * N + n] = (int16_t)mq;
        k_out[(uint64_t)c * N + n] = (uint8_t)kk;
        if (miu_out != nullptr) miu_out[n * C + c] = miu;
        if (sigma_out != nullptr) sigma_out[n * C + c] = sigma;
    }
}

__global__ void __launch_bounds__(GS_WAVE) gauss_ans_encode_kernel(uint64_t N, uint32_t S, uint32_t n_streams,
                                                                   const uint8_t *__restrict__ cm, const int16_t *__restrict__ mu_q,
                                                                   const uint8_t *__restrict__ k_lv, const uint16_t *__restrict__ G,
                                                                   uint8_t *__restrict__ scratch, uint32_t slot,
                                                                   uint32_t *__restrict__ lengths, uint32_t *__restrict__ states,
                                                                   uint32_t *__restrict__ status) {
    const uint32_t c = blockIdx.y;
    const uint32_t k = blockIdx.x * GS_WAVE + threadIdx.x;
    if (k >= n_streams) return;
    const AnsStream st = ans_stream(N, S, k, c, n_streams);
    const uint64_t base = (uint64_t)c * N + st.begin;
    uint8_t *dst = scratch + st.sid * slot;
    uint32_t pos = slot, x = ANS_L, bad = 0u;
    for (uint32_t i = st.len; i-- > 0u;) {
        const uint32_t s = cm[base + i];
        int32_t mq = mu_q[base + i];
        uint32_t kk = k_lv[base + i];
        if (mq < 0 || mq > GA_MU_MAX || kk >= GA_K) { // the host wrapper excludes it: keep the table index inside, report
            bad |= GA_STATUS_MODEL;
            mq = mq < 0 ? 0 : (mq > GA_MU_MAX ? GA_MU_MAX : mq);
            kk = kk >= GA_K ? GA_K - 1u : kk;
        }
        const uint32_t lo = ga_cum(G, kk, mq, s);
        ans_put(x, ga_cum(G, kk, mq, s + 1u) - lo, lo, GA_P, dst, pos, bad); // 1 <= f < 2^16
    }
    ans_finish(st.sid, slot - pos, x, bad, lengths, states, status);
}

__global__ void __launch_bounds__(GS_WAVE) gauss_ans_decode_kernel(uint64_t N, uint32_t C, uint32_t S, uint32_t n_streams,
                                                                   const uint8_t *__restrict__ payload, uint64_t payload_bytes,
                                                                   const int64_t *__restrict__ offsets, const int16_t *__restrict__ mu_q,
                                                                   const uint8_t *__restrict__ k_lv, const uint16_t *__restrict__ G,
                                                                   uint8_t *__restrict__ out) {
    const uint32_t c = blockIdx.y;
    const uint32_t k = blockIdx.x * GS_WAVE + threadIdx.x;
    if (k >= n_streams) return;
    const AnsStream st = ans_stream(N, S, k, c, n_streams);
    const uint64_t base = (uint64_t)c * N + st.begin;
    uint64_t rd, end;
    ans_range(payload_bytes, offsets, st.sid, rd, end);
    uint32_t x = 0u; // the 4 state bytes
#pragma unroll
    for (uint32_t b = 0u; b < 4u; ++b, ++rd) x |= ans_byte(payload, rd, end) << (8u * b);
    uint8_t *dst = out + st.begin * C + c;
    for (uint32_t i = 0u; i < st.len; ++i) {
        int32_t mq = mu_q[base + i];
        uint32_t kk = k_lv[base + i];
        mq = mq < 0 ? 0 : (mq > GA_MU_MAX ? GA_MU_MAX : mq);
        kk = kk >= GA_K ? GA_K - 1u : kk;
        const uint32_t sl = x & ((1u << GA_P) - 1u);
        uint32_t s = 0u; // the last s with cum(s) <= sl; s + step stays in 1..255
#pragma unroll
        for (uint32_t step = 128u; step >= 1u; step >>= 1)
            if (ga_cum_mid(G, kk, mq, s + step) <= sl) s += step;
        const uint32_t lo = ga_cum(G, kk, mq, s);
        x = ans_advance(x, ga_cum(G, kk, mq, s + 1u) - lo, lo, sl, GA_P, payload, rd, end);
        dst[(uint64_t)i * C] = (uint8_t)s;
    }
}

bool ga_shape_ok(uint64_t N, uint32_t C, uint32_t S) { return ans_shape_ok(N, C, S, GA_P, GA_MAX_C_CODER, GA_P, GA_P); }

template <int C>
void ga_params_launch(uint64_t N, const float *feat, const float *w1, const float *b1, const float *w2, const float *b2,
                      const float *mins, const float *maxs, const float *tau, int16_t *mu_q, uint8_t *k, float *miu, float *sigma,
                      hipStream_t st) {
    hipLaunchKernelGGL((gauss_ans_params_kernel<C>), dim3(gs_div_up(N, GS_BLOCK)), dim3(GS_BLOCK), 0, st, N, feat, w1, b1, w2, b2, mins,
                       maxs, tau, mu_q, k, miu, sigma);
}

} // namespace

extern "C" uint32_t gs_gauss_ans_slot_bytes(uint32_t S) { return ga_slot_bytes(S); }

extern "C" uint64_t gs_gauss_ans_encode_bytes(uint64_t N, uint32_t C, uint32_t S) {
    if (!ga_shape_ok(N, C, S)) return 0;
    return (uint64_t)C * ((N + S - 1) / S) * ga_slot_bytes(S);
}

extern "C" int32_t gs_gauss_ans_params(uint64_t N, uint32_t C, const float *features, const float *w1, const float *b1,
                                       const float *w2, const float *b2, const float *mins, const float *maxs,
                                       const float *thresholds, int16_t *mu_q, uint8_t *k, float *miu, float *sigma,
                                       gs_stream_t stream) {
    if (N == 0) return 0;
    GS_CHECK_ARG(C >= 1 && C <= GA_MAX_C, "1 <= channels <= 8");
    GS_CHECK_ARG(N < (1ull << 32), "too many splats for one launch");
    GS_CHECK_ARG(features && w1 && b1 && w2 && b2 && mins && maxs && thresholds && mu_q && k, "null pointer");
    GS_CHECK_ARG(((uintptr_t)features % 16u) == 0, "features must be 16-byte aligned");
    GS_CHECK_ARG(((uintptr_t)mu_q % 2u) == 0, "mu_q must be 2-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
#define GA_CASE(c)                                                                                           \
    case c:                                                                                                  \
        ga_params_launch<c>(N, features, w1, b1, w2, b2, mins, maxs, thresholds, mu_q, k, miu, sigma, st); \
        break;
    switch (C) {
        GA_CASE(1) GA_CASE(2) GA_CASE(3) GA_CASE(4) GA_CASE(5) GA_CASE(6) GA_CASE(7) GA_CASE(8)
    }
#undef GA_CASE
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_gauss_ans_encode(uint64_t N, uint32_t C, uint32_t S, const uint8_t *channel_major, const int16_t *mu_q,
                                       const uint8_t *k, const uint16_t *table, uint8_t *scratch, uint64_t scratch_bytes,
                                       uint32_t *lengths, uint32_t *states, uint32_t *status, gs_stream_t stream) {
    GS_CHECK_ARG(ga_shape_ok(N, C, S), "need 1 <= N < 2^32, 1 <= C <= 16, 1 <= S <= 2^24");
    GS_CHECK_ARG(channel_major && mu_q && k && table && scratch && lengths && states && status, "null pointer");
    GS_CHECK_ARG(((uintptr_t)mu_q % 2u) == 0 && ((uintptr_t)table % 2u) == 0, "mu_q and table must be 2-byte aligned");
    GS_CHECK_ARG(scratch_bytes >= gs_gauss_ans_encode_bytes(N, C, S), "scratch smaller than gs_gauss_ans_encode_bytes");
    const uint32_t n_streams = (uint32_t)((N + S - 1) / S);
    hipLaunchKernelGGL(gauss_ans_encode_kernel, dim3(gs_div_up(n_streams, GS_WAVE), C), dim3(GS_WAVE), 0, (hipStream_t)stream,
                       N, S, n_streams, channel_major, mu_q, k, table, scratch, ga_slot_bytes(S), lengths, states, status);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_gauss_ans_decode(uint64_t N, uint32_t C, uint32_t S, const uint8_t *payload, uint64_t payload_bytes,
                                       const int64_t *offsets, const int16_t *mu_q, const uint8_t *k, const uint16_t *table,
                                       uint8_t *symbols, gs_stream_t stream) {
    GS_CHECK_ARG(ga_shape_ok(N, C, S), "need 1 <= N < 2^32, 1 <= C <= 16, 1 <= S <= 2^24");
    GS_CHECK_ARG(payload && offsets && mu_q && k && table && symbols, "null pointer");
    GS_CHECK_ARG(((uintptr_t)mu_q % 2u) == 0 && ((uintptr_t)table % 2u) == 0, "mu_q and table must be 2-byte aligned");
    const uint32_t n_streams = (uint32_t)((N + S - 1) / S);
    hipLaunchKernelGGL(gauss_ans_decode_kernel, dim3(gs_div_up(n_streams, GS_WAVE), C), dim3(GS_WAVE), 0, (hipStream_t)stream, N, C, S,
                       n_streams, payload, payload_bytes, offsets, mu_q, k, table, symbols);
    GS_CHECK_LAUNCH();
    return 0;
}
