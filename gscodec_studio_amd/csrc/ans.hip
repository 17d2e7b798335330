// ans.hip -- the entropy coder of the on-disk format: static, table-based, byte-wise rANS over many independent streams (gfx950).
//
// The reference's EntropyCodingCompression (gsplat/compression/entropy_coding_compression.py:328-446) hands the 8-bit symbols of
// the scales and the quats to the `constriction` package, one categorical model per channel.  Here the coder is the library's
// own, and so is the bitstream: its definition is the numpy coder gscodec_studio_amd/compression/ans_reference.py, and every
// kernel below is integer arithmetic whose output is byte-identical to it.
//
// One stream -- state machine, geometry, slot writer, bounded reader -- is ans_stream_dev.h.  Here is the model: integer
// frequencies uint32 [C, 256] that sum to M = 2^P per channel (8 <= P <= 14) and their prefix sums, one LDS word per symbol, and for
// the decoder the table slot -> symbol (2^P bytes of LDS).  A lane emits at most ceil(S P / 8) + 1 bytes: a symbol costs
// log2(M / f) + log2(1 + 2^-9) bits at the most (the floor in x / f loses less than one part in 2^9 of a state >= 2^23 / 2^14), which
// is below P for every f >= 2 and exactly P for f = 1, and the state itself grows by less than 8 bits over the stream.
#include "ans_stream_dev.h"

namespace {

constexpr uint32_t ANS_MIN_P = 8, ANS_MAX_P = 14, ANS_MAX_C = 16, ANS_STATUS_ZERO_FREQ = 1u;
constexpr int ANS_ENC_BLOCK = GS_WAVE; // the encoder's tables are 1 KB: one wave per workgroup spreads the streams over the CUs

__host__ __device__ inline uint32_t ans_slot_bytes(uint32_t S, uint32_t P) { return (uint32_t)(((uint64_t)S * P + 7) / 8) + 8u; }

// symbols [N, C] -> counts [C, 256] (+ the channel-major copy [C, N]); n = N * C
__global__ void __launch_bounds__(GS_BLOCK) ans_histogram_kernel(uint64_t n, uint64_t N, uint32_t C, const uint8_t *__restrict__ sym,
                                                                 uint32_t *__restrict__ counts, uint8_t *__restrict__ cm) {
    __shared__ uint32_t s_hist[ANS_MAX_C * 256];
    for (uint32_t j = threadIdx.x; j < C * 256u; j += GS_BLOCK) s_hist[j] = 0u;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * GS_BLOCK;
    for (uint64_t i = (uint64_t)blockIdx.x * GS_BLOCK + threadIdx.x; i < n; i += stride) {
        const uint64_t r = i / C;
        const uint32_t c = (uint32_t)(i - r * C);
        const uint32_t s = sym[i];
        atomicAdd(&s_hist[c * 256u + s], 1u);
        if (cm != nullptr) cm[(uint64_t)c * N + r] = (uint8_t)s;
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < C * 256u; j += GS_BLOCK)
        if (s_hist[j] != 0u) atomicAdd(&counts[j], s_hist[j]);
}

// frequency (<= 2^14) in the high half, cumulative frequency (< 2^14) in the low half: one LDS read per symbol
GS_DEV uint32_t ans_pack_fc(uint32_t f, uint32_t c) { return (f << 16) | (c & 0xFFFFu); }

__global__ void __launch_bounds__(ANS_ENC_BLOCK) ans_encode_kernel(uint64_t N, uint32_t S, uint32_t P, uint32_t n_streams,
                                                                   const uint8_t *__restrict__ cm, const uint32_t *__restrict__ freq,
                                                                   const uint32_t *__restrict__ cum, uint8_t *__restrict__ scratch,
                                                                   uint32_t slot, uint32_t *__restrict__ lengths,
                                                                   uint32_t *__restrict__ states, uint32_t *__restrict__ status) {
    __shared__ uint32_t s_fc[256];
    const uint32_t c = blockIdx.y;
    for (uint32_t j = threadIdx.x; j < 256u; j += ANS_ENC_BLOCK) s_fc[j] = ans_pack_fc(freq[c * 256u + j], cum[c * 256u + j]);
    __syncthreads();
    const uint32_t k = blockIdx.x * ANS_ENC_BLOCK + threadIdx.x;
    if (k >= n_streams) return;
    const AnsStream st = ans_stream(N, S, k, c, n_streams);
    const uint8_t *src = cm + (uint64_t)c * N + st.begin;
    uint8_t *dst = scratch + st.sid * slot;
    uint32_t pos = slot, x = ANS_L, bad = 0u;
    for (uint32_t i = st.len; i-- > 0u;) {
        const uint32_t fc = s_fc[src[i]];
        uint32_t f = fc >> 16;
        if (f == 0u) { // a symbol the table does not have (the host wrapper excludes it): keep the division defined, report
            bad |= ANS_STATUS_ZERO_FREQ;
            f = 1u;
        }
        ans_put(x, f, fc & 0xFFFFu, P, dst, pos, bad);
    }
    ans_finish(st.sid, slot - pos, x, bad, lengths, states, status);
}

// one wave per stream: the little-endian final state, then the slot's bytes
__global__ void __launch_bounds__(GS_BLOCK) ans_pack_kernel(uint64_t n_total, uint32_t slot, const uint8_t *__restrict__ scratch,
                                                            const uint32_t *__restrict__ lengths, const uint32_t *__restrict__ states,
                                                            const int64_t *__restrict__ offsets, uint8_t *__restrict__ payload,
                                                            uint64_t payload_bytes) {
    const uint64_t sid = (uint64_t)blockIdx.x * (GS_BLOCK / GS_WAVE) + threadIdx.x / GS_WAVE;
    const uint32_t lane = threadIdx.x % GS_WAVE;
    if (sid >= n_total) return;
    const uint32_t len = lengths[sid] < slot ? lengths[sid] : slot;
    const int64_t off = offsets[sid];
    if (off < 0 || (uint64_t)off + 4u + len > payload_bytes) return;
    const uint8_t *src = scratch + (sid + 1) * slot - len;
    uint8_t *dst = payload + off;
    if (lane < 4u) dst[lane] = (uint8_t)((states[sid] >> (8u * lane)) & 0xFFu);
    for (uint32_t j = lane; j < len; j += GS_WAVE) dst[4u + j] = src[j];
}

__global__ void __launch_bounds__(GS_BLOCK) ans_decode_kernel(uint64_t N, uint32_t C, uint32_t S, uint32_t P, uint32_t n_streams,
                                                              const uint8_t *__restrict__ payload, uint64_t payload_bytes,
                                                              const int64_t *__restrict__ offsets, const uint32_t *__restrict__ freq,
                                                              const uint32_t *__restrict__ cum, uint8_t *__restrict__ out) {
    __shared__ uint32_t s_fc[256];
    __shared__ uint32_t s_cum[256];
    __shared__ uint8_t s_sym[1u << ANS_MAX_P];
    const uint32_t c = blockIdx.y;
    const uint32_t M = 1u << P;
    s_cum[threadIdx.x] = cum[c * 256u + threadIdx.x]; // GS_BLOCK == 256 symbols
    s_fc[threadIdx.x] = ans_pack_fc(freq[c * 256u + threadIdx.x], cum[c * 256u + threadIdx.x]);
    __syncthreads();
    // slot -> symbol: the LAST symbol whose cumulative frequency is <= slot (symbols of frequency 0 share their successor's)
    for (uint32_t sl = threadIdx.x; sl < M; sl += GS_BLOCK) {
        uint32_t lo = 0u;
#pragma unroll
        for (uint32_t step = 128u; step >= 1u; step >>= 1)
            if (s_cum[lo + step] <= sl) lo += step;
        s_sym[sl] = (uint8_t)lo;
    }
    __syncthreads();
    const uint32_t k = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (k >= n_streams) return;
    const AnsStream st = ans_stream(N, S, k, c, n_streams);
    uint64_t rd, end;
    ans_range(payload_bytes, offsets, st.sid, rd, end);
    uint32_t x = 0u; // the 4 state bytes
#pragma unroll
    for (uint32_t b = 0u; b < 4u; ++b, ++rd) x |= ans_byte(payload, rd, end) << (8u * b);
    uint8_t *dst = out + st.begin * C + c;
#pragma unroll 1 // every step waits for the state of the one before: a second copy of the body only costs registers
    for (uint32_t i = 0u; i < st.len; ++i) {
        const uint32_t sl = x & (M - 1u);
        const uint32_t s = s_sym[sl];
        const uint32_t fc = s_fc[s];
        x = ans_advance(x, fc >> 16, fc & 0xFFFFu, sl, P, payload, rd, end);
        dst[(uint64_t)i * C] = (uint8_t)s;
    }
}

bool ans_shape_ok(uint64_t N, uint32_t C, uint32_t S, uint32_t P) { return ans_shape_ok(N, C, S, P, ANS_MAX_C, ANS_MIN_P, ANS_MAX_P); }

} // namespace

extern "C" uint32_t gs_ans_slot_bytes(uint32_t S, uint32_t P) { return ans_slot_bytes(S, P); }

extern "C" uint64_t gs_ans_encode_bytes(uint64_t N, uint32_t C, uint32_t S, uint32_t P) {
    if (!ans_shape_ok(N, C, S, P)) return 0;
    return (uint64_t)C * ((N + S - 1) / S) * ans_slot_bytes(S, P);
}

extern "C" int32_t gs_ans_histogram(uint64_t N, uint32_t C, const uint8_t *symbols, uint32_t *counts, uint8_t *channel_major,
                                    gs_stream_t stream) {
    if (N == 0) return 0;
    GS_CHECK_ARG(symbols && counts, "null pointer");
    GS_CHECK_ARG(C >= 1 && C <= ANS_MAX_C, "1 <= channels <= 16");
    GS_CHECK_ARG(N < (1ull << 32), "too many symbols per channel for 32-bit counts");
    const uint64_t n = N * C;
    // 16 symbols per lane before another workgroup is opened: one flush of up to C * 256 atomics per workgroup
    const uint32_t blocks = (uint32_t)(gs_div_up(n, GS_BLOCK * 16) < 2048u ? gs_div_up(n, GS_BLOCK * 16) : 2048u);
    hipLaunchKernelGGL(ans_histogram_kernel, dim3(blocks), dim3(GS_BLOCK), 0, (hipStream_t)stream, n, N, C, symbols, counts, channel_major);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_ans_encode(uint64_t N, uint32_t C, uint32_t S, uint32_t P, const uint8_t *channel_major, const uint32_t *freq,
                                 const uint32_t *cum, uint8_t *scratch, uint64_t scratch_bytes, uint32_t *lengths, uint32_t *states,
                                 uint32_t *status, gs_stream_t stream) {
    GS_CHECK_ARG(ans_shape_ok(N, C, S, P), "need 1 <= N < 2^32, 1 <= C <= 16, 1 <= S <= 2^24, 8 <= P <= 14");
    GS_CHECK_ARG(channel_major && freq && cum && scratch && lengths && states && status, "null pointer");
    GS_CHECK_ARG(scratch_bytes >= gs_ans_encode_bytes(N, C, S, P), "scratch smaller than gs_ans_encode_bytes");
    const uint32_t n_streams = (uint32_t)((N + S - 1) / S);
    hipLaunchKernelGGL(ans_encode_kernel, dim3(gs_div_up(n_streams, ANS_ENC_BLOCK), C), dim3(ANS_ENC_BLOCK), 0, (hipStream_t)stream, N, S,
                       P, n_streams, channel_major, freq, cum, scratch, ans_slot_bytes(S, P), lengths, states, status);
    GS_CHECK_LAUNCH();
    return 0;
}

// the pack launch, for either model: the slot size is an argument; gs_ans_pack gives it as this file's (S, P)
extern "C" int32_t gs_ans_pack_slots(uint64_t n_streams_total, uint32_t slot_bytes, const uint8_t *scratch, const uint32_t *lengths,
                                     const uint32_t *states, const int64_t *offsets, uint8_t *payload, uint64_t payload_bytes,
                                     gs_stream_t stream) {
    if (n_streams_total == 0) return 0;
    GS_CHECK_ARG(scratch && lengths && states && offsets && payload, "null pointer");
    GS_CHECK_ARG(slot_bytes >= 1, "slot_bytes must be positive");
    const uint32_t blocks = gs_div_up(n_streams_total, GS_BLOCK / GS_WAVE); // a wave per stream
    GS_CHECK_ARG(blocks < (1ull << 31), "too many streams");
    hipLaunchKernelGGL(ans_pack_kernel, dim3(blocks), dim3(GS_BLOCK), 0, (hipStream_t)stream, n_streams_total, slot_bytes, scratch,
                       lengths, states, offsets, payload, payload_bytes);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_ans_pack(uint64_t n_streams_total, uint32_t S, uint32_t P, const uint8_t *scratch, const uint32_t *lengths,
                               const uint32_t *states, const int64_t *offsets, uint8_t *payload, uint64_t payload_bytes,
                               gs_stream_t stream) {
    if (n_streams_total == 0) return 0;
    GS_CHECK_ARG(scratch && lengths && states && offsets && payload, "null pointer");
    GS_CHECK_ARG(S >= 1 && S <= (1u << 24) && P >= ANS_MIN_P && P <= ANS_MAX_P, "need 1 <= S <= 2^24, 8 <= P <= 14");
    return gs_ans_pack_slots(n_streams_total, ans_slot_bytes(S, P), scratch, lengths, states, offsets, payload, payload_bytes, stream);
}

extern "C" int32_t gs_ans_decode(uint64_t N, uint32_t C, uint32_t S, uint32_t P, const uint8_t *payload, uint64_t payload_bytes,
                                 const int64_t *offsets, const uint32_t *freq, const uint32_t *cum, uint8_t *symbols,
                                 gs_stream_t stream) {
    GS_CHECK_ARG(ans_shape_ok(N, C, S, P), "need 1 <= N < 2^32, 1 <= C <= 16, 1 <= S <= 2^24, 8 <= P <= 14");
    GS_CHECK_ARG(payload && offsets && freq && cum && symbols, "null pointer");
    const uint32_t n_streams = (uint32_t)((N + S - 1) / S);
    hipLaunchKernelGGL(ans_decode_kernel, dim3(gs_div_up(n_streams, GS_BLOCK), C), dim3(GS_BLOCK), 0, (hipStream_t)stream, N, C, S, P,
                       n_streams, payload, payload_bytes, offsets, freq, cum, symbols);
    GS_CHECK_LAUNCH();
    return 0;
}
