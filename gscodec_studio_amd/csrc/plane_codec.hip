// plane_codec.hip -- the transform-coded attribute planes of HevcCompression: a small intra codec for 8-bit planes [H, W, ch] with
// HEVC's quantisation parameter (gfx950).
//
// The reference's HevcCompression (gsplat/compression/hevc_compression.py) shells out to ffmpeg / libx265 and reads the .mp4 back.
// Here the payload is the library's own bitstream: its definition is the numpy module
// gscodec_studio_amd/compression/plane_codec_reference.py, and every kernel below computes what that module computes -- integer
// arithmetic only, so levels, planes and bytes are equal, not close.  It is no HEVC stream: HEVC's 8-point transform and flat
// quantiser (so that qp keeps its meaning), no prediction, no RDO, rANS over 15 static tables in place of CABAC.
//
// plane_fwd_kernel / plane_inv_kernel: ONE LANE OWNS ONE 8 x 8 BLOCK of one image channel.  The block, the intermediate and the
//   coefficients are fully unrolled int32 arrays in registers (no LDS, no scratch: csrc/resources.sh gives 94 / 138 VGPRs and scratch 0); the
//   matrix is immediates.  The forward reads its 64 bytes with clamped coordinates (the edge replication of the padding) and stores
//   its 64 int16 levels in scan order as eight 16-byte words; the inverse clamps the levels, and stores only the pixels inside the
//   plane (the crop).  47,628 blocks for three channels of a million splats: 745 waves, once per file.
// plane_seq_fwd_kernel / plane_seq_inv_kernel: the closed loop of SeqHevcCompression's plane sequences (the numpy module
//   plane_seq_codec_reference.py defines it) in ONE launch: a lane owns its block through all T frames.  The stages are the same
//   device functions as the per-plane kernels' (pc_load_pixels, pc_forward, pc_store_levels, pc_load_coefs / pc_dequant, pc_inverse,
//   pc_store_pixels); what is added is the state -- the padded reconstruction, 64 bytes in 16 registers, never in memory -- and, in
//   the forward, the next frame's 64 source bytes: their loads are issued at the top of an iteration into registers that nothing
//   reads before the state update at its end, so the compiled loop has the 64 global_load_ubyte in front of the forward transform
//   and its only wait for them at the loop's back edge, behind both transforms (read in the ISA, not assumed from the source order).
//   Scratch 0 for both; the forward holds the state, this frame, the frame in flight and both transforms' working sets and runs at
//   one wave per SIMD (256 VGPRs + 224 AGPRs), which costs nothing here: three channels of a million splats are 745 waves for 1024
//   SIMDs.  The inverse needs no such care: the levels of every frame are independent of the state.
// plane_ans_encode_kernel / plane_ans_decode_kernel: ans_stream_dev.h's streams, one lane per stream, over the flat symbol
//   sequence as ONE channel; the model of symbol i is the table of context CTX[i % 64] (the anti-diagonal of its scan position), the
//   15 cumulative tables (uint16 [15][257], 7.7 KB) live in LDS.  The decoder's 8-step binary search has a fixed trip count and its
//   reads are ans_range / ans_byte's: a damaged stream decodes to wrong symbols, nothing else.
#include "ans_stream_dev.h"

namespace {

constexpr uint32_t PC_CONTEXTS = 15, PC_CUM_ROW = 257, PC_MAX_CH = 4, PC_MAX_QP = 51, PC_MIN_P = 8, PC_MAX_P = 14;
constexpr int32_t PC_LEVEL_MAX = 32767;
constexpr uint32_t PC_STATUS_MODEL = 1u;

// scan position k -> the coefficient at row i (vertical frequency), column j, as 8 i + j: by anti-diagonal i + j, ascending i inside
#define PC_SCAN_TABLE                                                                                                              \
    {0, 1, 8, 2, 9, 16, 3, 10, 17, 24, 4, 11, 18, 25, 32, 5, 12, 19, 26, 33, 40, 6, 13, 20, 27, 34, 41, 48, 7, 14, 21, 28, 35, 42, 49, \
     56, 15, 22, 29, 36, 43, 50, 57, 23, 30, 37, 44, 51, 58, 31, 38, 45, 52, 59, 39, 46, 53, 60, 47, 54, 61, 55, 62, 63}
#define PC_MATRIX                                                                                                            \
    {{64, 64, 64, 64, 64, 64, 64, 64}, {89, 75, 50, 18, -18, -50, -75, -89}, {83, 36, -36, -83, -83, -36, 36, 83},           \
     {75, -18, -89, -50, 50, 89, 18, -75}, {64, -64, -64, 64, 64, -64, -64, 64}, {50, -89, 18, 75, -75, -18, 89, -50},       \
     {36, -83, 83, -36, -36, 83, -83, 36}, {18, -50, 75, -89, 89, -75, 50, -18}}

GS_DEV int32_t pc_rs(int32_t v, int32_t s) { return (v + (1 << (s - 1))) >> s; }
GS_DEV int32_t pc_clip(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// out[u] = sum_x M[u][x] in[x] (the forward direction), or out[x] = sum_u M[u][x] in[u] (TRANSPOSED: the inverse)
template <bool TRANSPOSED>
GS_DEV void pc_mul8(const int32_t (&in)[8], int32_t (&out)[8]) {
    constexpr int32_t M[8][8] = PC_MATRIX;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        int32_t acc = 0;
#pragma unroll
        for (int b = 0; b < 8; ++b) acc += (TRANSPOSED ? M[b][a] : M[a][b]) * in[b];
        out[a] = acc;
    }
}

struct PcGeom { uint32_t H, W, ch, bw, n_blocks; };

// ---- the stages: ONE definition each, shared by the per-plane kernels and the sequence kernels below.  A block is int32 [64] in
// registers, pixel (y, x) or coefficient (v, u) at 8 y + x / 8 v + u; every loop is fully unrolled.

// the 64 source bytes of block (y0, x0) of channel c, coordinates clamped into the plane: the edge replication of the padding
GS_DEV void pc_load_pixels(const PcGeom &g, uint32_t c, uint32_t y0, uint32_t x0, const uint8_t *__restrict__ plane, int32_t (&px)[64]) {
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        const uint32_t yy = min(y0 + (uint32_t)y, g.H - 1u);
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const uint32_t xx = min(x0 + (uint32_t)x, g.W - 1u);
            px[y * 8 + x] = plane[((uint64_t)yy * g.W + xx) * g.ch + c];
        }
    }
}

// the pixels inside the plane (the crop); px in 0..255
GS_DEV void pc_store_pixels(const PcGeom &g, uint32_t c, uint32_t y0, uint32_t x0, const int32_t (&px)[64], uint8_t *__restrict__ plane) {
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        const uint32_t yy = y0 + (uint32_t)y;
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const uint32_t xx = x0 + (uint32_t)x;
            if (yy < g.H && xx < g.W) plane[((uint64_t)yy * g.W + xx) * g.ch + c] = (uint8_t)px[y * 8 + x];
        }
    }
}

// forward transform (along x with rs(., 2), then along y with rs(., 9)) and quantiser of a block of pixels (0..255) or of
// residuals (-255..255): |sum over a row of M| <= 512 per pass, so |row| <= 512 * 255 < 2^17, |t| <= 32640, |column| <= 512 * 32640
// < 2^24 and |coef| <= 32640 for either input
GS_DEV void pc_forward(const int32_t (&px)[64], uint32_t qp, int32_t (&level)[64]) {
    constexpr uint32_t QS[6] = {26214u, 23302u, 20560u, 18396u, 16384u, 14564u};
    int32_t t[8][8]; // [y][u]
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        int32_t in[8], row[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) in[x] = px[y * 8 + x];
        pc_mul8<false>(in, row);
#pragma unroll
        for (int u = 0; u < 8; ++u) t[y][u] = pc_rs(row[u], 2);
    }
    const uint32_t qbits = 18u + qp / 6u, qs = QS[qp % 6u], round = 171u << (qbits - 9u);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        int32_t col[8], out[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) col[y] = t[y][u];
        pc_mul8<false>(col, out);
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const int32_t coef = pc_rs(out[v], 9); // |coef| <= 32640: the product below stays under 2^30
            const uint32_t mag = ((uint32_t)(coef < 0 ? -coef : coef) * qs + round) >> qbits;
            level[v * 8 + u] = coef < 0 ? -(int32_t)mag : (int32_t)mag;
        }
    }
}

// the 64 levels of a block in scan order as eight 16-byte words (128 bytes per block: aligned with the buffer)
GS_DEV void pc_store_levels(const int32_t (&level)[64], int16_t *__restrict__ dst16) {
    constexpr uint8_t SCAN[64] = PC_SCAN_TABLE;
    uint4 *dst = reinterpret_cast<uint4 *>(dst16);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        uint32_t w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            w[e] = ((uint32_t)level[SCAN[q * 8 + e * 2]] & 0xFFFFu) | ((uint32_t)level[SCAN[q * 8 + e * 2 + 1]] << 16);
        dst[q] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// the dequantiser scale of a qp: LS[qp % 6] << (qp / 6) <= 72 * 256
GS_DEV int32_t pc_scale(uint32_t qp) {
    constexpr int32_t LS[6] = {40, 45, 51, 57, 64, 72};
    return LS[qp % 6u] * (1 << (qp / 6u));
}

// dequantiser: the level clamped to +-32767, times the scale (<= 72 * 256: it fits int32), rounded, clipped to int16
GS_DEV int32_t pc_dequant(int32_t level, int32_t scale) {
    return pc_clip((pc_clip(level, -PC_LEVEL_MAX, PC_LEVEL_MAX) * scale + 2) >> 2, -32768, 32767);
}

// the 64 stored levels of a block (any int16 values), out of scan order, dequantised: coef [v][u]
GS_DEV void pc_load_coefs(const int16_t *__restrict__ src16, int32_t scale, int32_t (&coef)[64]) {
    constexpr uint8_t SCAN[64] = PC_SCAN_TABLE;
    const uint4 *src = reinterpret_cast<const uint4 *>(src16);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint4 v4 = src[q];
        const uint32_t w[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            coef[SCAN[q * 8 + e * 2]] = pc_dequant((int32_t)(int16_t)(w[e] & 0xFFFFu), scale);
            coef[SCAN[q * 8 + e * 2 + 1]] = pc_dequant((int32_t)w[e] >> 16, scale);
        }
    }
}

// inverse transform of int16 coefficients: along y with rs(., 7) and the int16 clip (|column| <= 512 * 32768 = 2^24), then along
// x with rs(., 12) (|row| <= 2^24 again).  NOT clipped to 0..255: a frame clips it, a residual is added to the prediction first
GS_DEV void pc_inverse(const int32_t (&coef)[64], int32_t (&px)[64]) {
    int32_t t[8][8]; // [y][u]
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        int32_t col[8], out[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) col[v] = coef[v * 8 + u];
        pc_mul8<true>(col, out);
#pragma unroll
        for (int y = 0; y < 8; ++y) t[y][u] = pc_clip(pc_rs(out[y], 7), -32768, 32767);
    }
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        int32_t out[8];
        pc_mul8<true>(t[y], out);
#pragma unroll
        for (int x = 0; x < 8; ++x) px[y * 8 + x] = pc_rs(out[x], 12);
    }
}

__global__ void __launch_bounds__(GS_BLOCK) plane_fwd_kernel(PcGeom g, uint32_t qp, const uint8_t *__restrict__ plane,
                                                             int16_t *__restrict__ levels) {
    const uint32_t gid = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (gid >= g.ch * g.n_blocks) return;
    const uint32_t c = gid / g.n_blocks, b = gid - c * g.n_blocks;
    int32_t px[64], level[64];
    pc_load_pixels(g, c, (b / g.bw) * 8u, (b % g.bw) * 8u, plane, px);
    pc_forward(px, qp, level);
    pc_store_levels(level, levels + (uint64_t)gid * 64u);
}

__global__ void __launch_bounds__(GS_BLOCK) plane_inv_kernel(PcGeom g, uint32_t qp, const int16_t *__restrict__ levels,
                                                             uint8_t *__restrict__ plane) {
    const uint32_t gid = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (gid >= g.ch * g.n_blocks) return;
    const uint32_t c = gid / g.n_blocks, b = gid - c * g.n_blocks;
    int32_t coef[64], px[64];
    pc_load_coefs(levels + (uint64_t)gid * 64u, pc_scale(qp), coef);
    pc_inverse(coef, px);
#pragma unroll
    for (int i = 0; i < 64; ++i) px[i] = pc_clip(px[i], 0, 255);
    pc_store_pixels(g, c, (b / g.bw) * 8u, (b % g.bw) * 8u, px, plane);
}

// ---- the sequence kernels: one lane owns one block of one channel through all T frames.  The padded reconstruction (the state
// of the format: 64 values in 0..255) stays in registers, four pixels to a word.
GS_DEV int32_t pc_byte(const uint32_t (&packed)[16], int i) { return (int32_t)((packed[i >> 2] >> (8 * (i & 3))) & 0xFFu); }

GS_DEV void pc_pack(const int32_t (&px)[64], uint32_t (&packed)[16]) {
#pragma unroll
    for (int w = 0; w < 16; ++w)
        packed[w] = (uint32_t)px[4 * w] | ((uint32_t)px[4 * w + 1] << 8) | ((uint32_t)px[4 * w + 2] << 16) | ((uint32_t)px[4 * w + 3] << 24);
}

// state <- clip(prediction + residual, 0, 255) with prediction = 0 on an I frame (keep = 0) and the state on a P frame (keep = ~0);
// px leaves as the new state's values
GS_DEV void pc_update_state(uint32_t keep, int32_t (&px)[64], uint32_t (&state)[16]) {
#pragma unroll
    for (int i = 0; i < 64; ++i) px[i] = pc_clip((int32_t)((uint32_t)pc_byte(state, i) & keep) + px[i], 0, 255);
    pc_pack(px, state);
}

__global__ void __launch_bounds__(GS_BLOCK) plane_seq_fwd_kernel(PcGeom g, uint32_t T, uint32_t gop, uint32_t qp,
                                                                 const uint8_t *__restrict__ planes, int16_t *__restrict__ levels,
                                                                 uint8_t *__restrict__ recon) {
    const uint32_t gid = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (gid >= g.ch * g.n_blocks) return;
    const uint32_t c = gid / g.n_blocks, b = gid - c * g.n_blocks;
    const uint32_t y0 = (b / g.bw) * 8u, x0 = (b % g.bw) * 8u;
    const uint64_t frame = (uint64_t)g.H * g.W * g.ch, frame_levels = (uint64_t)g.ch * g.n_blocks * 64u;
    const int32_t scale = pc_scale(qp);
    uint32_t state[16];
    int32_t cur[64]; // this frame's source bytes, one to a register: loaded an iteration ahead
#pragma unroll
    for (int w = 0; w < 16; ++w) state[w] = 0u;
    pc_load_pixels(g, c, y0, x0, planes, cur);
    for (uint32_t t = 0u; t < T; ++t) {
        const uint32_t keep = (t % gop == 0u) ? 0u : ~0u;
        int32_t px[64], ahead[64];
#pragma unroll
        for (int i = 0; i < 64; ++i) px[i] = cur[i] - (int32_t)((uint32_t)pc_byte(state, i) & keep); // -255..255
        // the next frame's bytes: requested here, first read behind the state update at the end of the iteration, so that the wait
        // for them falls behind both transforms (behind the last frame the frame itself is loaded again: in bounds, not used)
        pc_load_pixels(g, c, y0, x0, planes + (uint64_t)min(t + 1u, T - 1u) * frame, ahead);
        int32_t level[64];
        pc_forward(px, qp, level);
        pc_store_levels(level, levels + (uint64_t)t * frame_levels + (uint64_t)gid * 64u);
#pragma unroll
        for (int i = 0; i < 64; ++i) level[i] = pc_dequant(level[i], scale);
        pc_inverse(level, px);
        pc_update_state(keep, px, state);
        if (recon) pc_store_pixels(g, c, y0, x0, px, recon + (uint64_t)t * frame);
#pragma unroll
        for (int i = 0; i < 64; ++i) cur[i] = ahead[i];
    }
}

__global__ void __launch_bounds__(GS_BLOCK) plane_seq_inv_kernel(PcGeom g, uint32_t T, uint32_t gop, uint32_t qp,
                                                                 const int16_t *__restrict__ levels, uint8_t *__restrict__ planes) {
    const uint32_t gid = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (gid >= g.ch * g.n_blocks) return;
    const uint32_t c = gid / g.n_blocks, b = gid - c * g.n_blocks;
    const uint32_t y0 = (b / g.bw) * 8u, x0 = (b % g.bw) * 8u;
    const uint64_t frame = (uint64_t)g.H * g.W * g.ch, frame_levels = (uint64_t)g.ch * g.n_blocks * 64u;
    const int32_t scale = pc_scale(qp);
    uint32_t state[16];
#pragma unroll
    for (int w = 0; w < 16; ++w) state[w] = 0u;
    for (uint32_t t = 0u; t < T; ++t) { // the levels of every frame are independent of the state: the loads run ahead by themselves
        int32_t coef[64], px[64];
        pc_load_coefs(levels + (uint64_t)t * frame_levels + (uint64_t)gid * 64u, scale, coef);
        pc_inverse(coef, px);
        pc_update_state((t % gop == 0u) ? 0u : ~0u, px, state);
        pc_store_pixels(g, c, y0, x0, px, planes + (uint64_t)t * frame);
    }
}

// the 15 cumulative tables and the context of a scan position, into LDS (every lane of the workgroup calls it)
GS_DEV void pc_load_model(const uint16_t *__restrict__ cum, uint16_t *s_cum, uint8_t *s_ctx) {
    constexpr uint8_t SCAN[64] = PC_SCAN_TABLE;
    for (uint32_t j = threadIdx.x; j < PC_CONTEXTS * PC_CUM_ROW; j += GS_WAVE) s_cum[j] = cum[j];
    if (threadIdx.x < 64u) s_ctx[threadIdx.x] = (uint8_t)((SCAN[threadIdx.x] >> 3) + (SCAN[threadIdx.x] & 7u));
    __syncthreads();
}

__global__ void __launch_bounds__(GS_WAVE) plane_ans_encode_kernel(uint64_t N, uint32_t S, uint32_t P, uint32_t n_streams,
                                                                   const uint8_t *__restrict__ symbols, const uint16_t *__restrict__ cum,
                                                                   uint8_t *__restrict__ scratch, uint32_t slot,
                                                                   uint32_t *__restrict__ lengths, uint32_t *__restrict__ states,
                                                                   uint32_t *__restrict__ status) {
    __shared__ uint16_t s_cum[PC_CONTEXTS * PC_CUM_ROW];
    __shared__ uint8_t s_ctx[64];
    pc_load_model(cum, s_cum, s_ctx);
    const uint32_t k = blockIdx.x * GS_WAVE + threadIdx.x;
    if (k >= n_streams) return;
    const AnsStream st = ans_stream(N, S, k, 0u, n_streams);
    uint8_t *dst = scratch + st.sid * slot;
    uint32_t pos = slot, x = ANS_L, bad = 0u;
    for (uint32_t i = st.len; i-- > 0u;) {
        const uint64_t at = st.begin + i;
        const uint32_t row = (uint32_t)s_ctx[at & 63u] * PC_CUM_ROW + symbols[at];
        const uint32_t lo = s_cum[row];
        uint32_t f = (uint32_t)s_cum[row + 1u] - lo;
        if (f == 0u || f > (1u << P)) { // the host wrapper excludes it (the tables come from these symbols' histogram): report
            bad |= PC_STATUS_MODEL;
            f = 1u;
        }
        ans_put(x, f, lo, P, dst, pos, bad);
    }
    ans_finish(st.sid, slot - pos, x, bad, lengths, states, status);
}

__global__ void __launch_bounds__(GS_WAVE) plane_ans_decode_kernel(uint64_t N, uint32_t S, uint32_t P, uint32_t n_streams,
                                                                   const uint8_t *__restrict__ payload, uint64_t payload_bytes,
                                                                   const int64_t *__restrict__ offsets, const uint16_t *__restrict__ cum,
                                                                   uint8_t *__restrict__ out) {
    __shared__ uint16_t s_cum[PC_CONTEXTS * PC_CUM_ROW];
    __shared__ uint8_t s_ctx[64];
    pc_load_model(cum, s_cum, s_ctx);
    const uint32_t k = blockIdx.x * GS_WAVE + threadIdx.x;
    if (k >= n_streams) return;
    const AnsStream st = ans_stream(N, S, k, 0u, n_streams);
    uint64_t rd, end;
    ans_range(payload_bytes, offsets, st.sid, rd, end);
    uint32_t x = 0u; // the 4 state bytes
#pragma unroll
    for (uint32_t b = 0u; b < 4u; ++b, ++rd) x |= ans_byte(payload, rd, end) << (8u * b);
    for (uint32_t i = 0u; i < st.len; ++i) {
        const uint64_t at = st.begin + i;
        const uint16_t *row = s_cum + (uint32_t)s_ctx[at & 63u] * PC_CUM_ROW;
        const uint32_t sl = x & ((1u << P) - 1u);
        uint32_t s = 0u; // the last s with cum(s) <= sl; s + step stays in 1..255
#pragma unroll
        for (uint32_t step = 128u; step >= 1u; step >>= 1)
            if ((uint32_t)row[s + step] <= sl) s += step;
        const uint32_t lo = row[s];
        x = ans_advance(x, (uint32_t)row[s + 1u] - lo, lo, sl, P, payload, rd, end);
        out[at] = (uint8_t)s;
    }
}

bool pc_plane_ok(uint32_t H, uint32_t W, uint32_t ch, uint32_t qp) {
    if (H < 1u || W < 1u || ch < 1u || ch > PC_MAX_CH || qp > PC_MAX_QP) return false;
    return (uint64_t)((H + 7u) / 8u) * ((W + 7u) / 8u) * ch * 64u < (1ull << 31);
}

PcGeom pc_geom(uint32_t H, uint32_t W, uint32_t ch) {
    const uint32_t bw = (W + 7u) / 8u;
    return {H, W, ch, bw, bw * ((H + 7u) / 8u)};
}

} // namespace

extern "C" uint32_t gs_plane_ans_slot_bytes(uint32_t S, uint32_t P) { return (uint32_t)(((uint64_t)S * P + 7u) / 8u) + 8u; }

extern "C" int32_t gs_plane_transform_fwd(uint32_t H, uint32_t W, uint32_t ch, uint32_t qp, const uint8_t *plane, int16_t *levels,
                                          gs_stream_t stream) {
    GS_CHECK_ARG(pc_plane_ok(H, W, ch, qp), "need H, W >= 1, 1 <= ch <= 4, qp <= 51 and fewer than 2^31 coefficients");
    GS_CHECK_ARG(plane && levels, "null pointer");
    GS_CHECK_ARG(((uintptr_t)levels % 16u) == 0, "levels must be 16-byte aligned");
    const PcGeom g = pc_geom(H, W, ch);
    hipLaunchKernelGGL(plane_fwd_kernel, dim3(gs_div_up((uint64_t)g.ch * g.n_blocks, GS_BLOCK)), dim3(GS_BLOCK), 0, (hipStream_t)stream, g,
                       qp, plane, levels);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_plane_transform_inv(uint32_t H, uint32_t W, uint32_t ch, uint32_t qp, const int16_t *levels, uint8_t *plane,
                                          gs_stream_t stream) {
    GS_CHECK_ARG(pc_plane_ok(H, W, ch, qp), "need H, W >= 1, 1 <= ch <= 4, qp <= 51 and fewer than 2^31 coefficients");
    GS_CHECK_ARG(plane && levels, "null pointer");
    GS_CHECK_ARG(((uintptr_t)levels % 16u) == 0, "levels must be 16-byte aligned");
    const PcGeom g = pc_geom(H, W, ch);
    hipLaunchKernelGGL(plane_inv_kernel, dim3(gs_div_up((uint64_t)g.ch * g.n_blocks, GS_BLOCK)), dim3(GS_BLOCK), 0, (hipStream_t)stream, g,
                       qp, levels, plane);
    GS_CHECK_LAUNCH();
    return 0;
}

namespace {
bool pc_seq_ok(uint32_t T, uint32_t gop, uint32_t H, uint32_t W, uint32_t ch, uint32_t qp) {
    if (T < 1u || gop < 1u || !pc_plane_ok(H, W, ch, qp)) return false;
    return (uint64_t)T * ((H + 7u) / 8u) * ((W + 7u) / 8u) * ch * 64u < (1ull << 31); // < 2^31 per frame: the product fits uint64
}
} // namespace

extern "C" int32_t gs_plane_seq_fwd(uint32_t T, uint32_t gop, uint32_t H, uint32_t W, uint32_t ch, uint32_t qp, const uint8_t *planes,
                                    int16_t *levels, uint8_t *recon, gs_stream_t stream) {
    GS_CHECK_ARG(pc_seq_ok(T, gop, H, W, ch, qp), "need T, gop, H, W >= 1, 1 <= ch <= 4, qp <= 51 and fewer than 2^31 coefficients");
    GS_CHECK_ARG(planes && levels, "null pointer");
    GS_CHECK_ARG(((uintptr_t)levels % 16u) == 0, "levels must be 16-byte aligned");
    const PcGeom g = pc_geom(H, W, ch);
    hipLaunchKernelGGL(plane_seq_fwd_kernel, dim3(gs_div_up((uint64_t)g.ch * g.n_blocks, GS_BLOCK)), dim3(GS_BLOCK), 0, (hipStream_t)stream,
                       g, T, gop, qp, planes, levels, recon);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_plane_seq_inv(uint32_t T, uint32_t gop, uint32_t H, uint32_t W, uint32_t ch, uint32_t qp, const int16_t *levels,
                                    uint8_t *planes, gs_stream_t stream) {
    GS_CHECK_ARG(pc_seq_ok(T, gop, H, W, ch, qp), "need T, gop, H, W >= 1, 1 <= ch <= 4, qp <= 51 and fewer than 2^31 coefficients");
    GS_CHECK_ARG(planes && levels, "null pointer");
    GS_CHECK_ARG(((uintptr_t)levels % 16u) == 0, "levels must be 16-byte aligned");
    const PcGeom g = pc_geom(H, W, ch);
    hipLaunchKernelGGL(plane_seq_inv_kernel, dim3(gs_div_up((uint64_t)g.ch * g.n_blocks, GS_BLOCK)), dim3(GS_BLOCK), 0, (hipStream_t)stream,
                       g, T, gop, qp, levels, planes);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_plane_ans_encode(uint64_t N, uint32_t S, uint32_t P, const uint8_t *symbols, const uint16_t *cum, uint8_t *scratch,
                                       uint64_t scratch_bytes, uint32_t *lengths, uint32_t *states, uint32_t *status,
                                       gs_stream_t stream) {
    GS_CHECK_ARG(ans_shape_ok(N, 1u, S, P, 1u, PC_MIN_P, PC_MAX_P) && N % 64u == 0, "need N a multiple of 64 below 2^32, 1 <= S <= 2^24, 8 <= P <= 14");
    GS_CHECK_ARG(symbols && cum && scratch && lengths && states && status, "null pointer");
    GS_CHECK_ARG(((uintptr_t)cum % 2u) == 0, "cum must be 2-byte aligned");
    const uint32_t n_streams = (uint32_t)((N + S - 1) / S);
    GS_CHECK_ARG(scratch_bytes >= (uint64_t)n_streams * gs_plane_ans_slot_bytes(S, P), "scratch smaller than n_streams * gs_plane_ans_slot_bytes");
    hipLaunchKernelGGL(plane_ans_encode_kernel, dim3(gs_div_up(n_streams, GS_WAVE)), dim3(GS_WAVE), 0, (hipStream_t)stream, N, S, P,
                       n_streams, symbols, cum, scratch, gs_plane_ans_slot_bytes(S, P), lengths, states, status);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_plane_ans_decode(uint64_t N, uint32_t S, uint32_t P, const uint8_t *payload, uint64_t payload_bytes,
                                       const int64_t *offsets, const uint16_t *cum, uint8_t *symbols, gs_stream_t stream) {
    GS_CHECK_ARG(ans_shape_ok(N, 1u, S, P, 1u, PC_MIN_P, PC_MAX_P) && N % 64u == 0, "need N a multiple of 64 below 2^32, 1 <= S <= 2^24, 8 <= P <= 14");
    GS_CHECK_ARG(payload && offsets && cum && symbols, "null pointer");
    GS_CHECK_ARG(((uintptr_t)cum % 2u) == 0, "cum must be 2-byte aligned");
    const uint32_t n_streams = (uint32_t)((N + S - 1) / S);
    hipLaunchKernelGGL(plane_ans_decode_kernel, dim3(gs_div_up(n_streams, GS_WAVE)), dim3(GS_WAVE), 0, (hipStream_t)stream, N, S, P,
                       n_streams, payload, payload_bytes, offsets, cum, symbols);
    GS_CHECK_LAUNCH();
    return 0;
}
