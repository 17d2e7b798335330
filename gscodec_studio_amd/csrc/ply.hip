// ply.hip -- the vertex rows of a binary little-endian .ply (the INRIA 3DGS layout and its relatives) to and from the six splat
// tensors (gfx950).
//
// The reference reads and writes such files on the host through the plyfile package (examples/simple_trainer.py:414-510: one
// Python tuple per splat on the way out, 62 float64 column copies on the way in).  Here the raw rows travel to the GPU as they
// are and one kernel transposes them:
//
//   gs_ply_unpack   rows -> means, sh0, shN, opacities, scales, quats, optionally with the trainer's activations and the
//                   quaternion normalisation (the rasterizer's inputs, as gs_decode_splats gives them)
//   gs_ply_pack     the six tensors -> rows; bytes of a row that no column covers (the normals) are zero
//
// A workgroup of 256 lanes owns R consecutive rows (R = 256, 128 or 64: the largest whose R * stride bytes fit the 64 KB of
// LDS it stages them in).  The block's bytes are one contiguous run of the file, moved with 16-byte global accesses; every
// tensor is then written (read) as the flat element range [row0 * W, (row0 + count) * W), lane k next to lane k + 1, and the LDS
// takes the scatter.  Which byte of a row an output element comes from is a table the host builds from the file's header: one
// entry per output element of a row, in output order, so the channel-major f_dc_* / f_rest_* columns become [K, 3] through the
// table and the kernel knows nothing of names or orders.  Nothing here is arithmetic except the activations
// (decode_act_dev.h, shared with gs_decode_splats) and the rounding of a `double` column to float.
#include "gs_common.h"
#include "decode_act_dev.h"

namespace {

constexpr uint32_t PLY_MAX_STRIDE = 1024;  // bytes per row: 64 rows of it fill the LDS
constexpr uint32_t PLY_MAX_COLUMNS = 128;  // table entries: 3 + 3 + 3 * 24 + 1 + 3 + 4 = 86 at SH degree 4
constexpr uint32_t PLY_LDS_BYTES = 65536;
constexpr uint32_t PLY_GROUPS = 6;         // means, sh0, shN, opacities, scales, quats
constexpr uint32_t PLY_OFFSET_MASK = 0xFFFFu, PLY_DOUBLE = 1u << 16;

enum { PLY_ACT_NONE = 0, PLY_ACT_EXP = 1, PLY_ACT_SIGMOID = 2, PLY_ACT_NORMALIZE = 3 };

struct PlyTable {
    uint32_t col[PLY_MAX_COLUMNS]; // byte offset inside the row | PLY_DOUBLE, per element of a row of group 0, 1, ...
    float *ptr[PLY_GROUPS];        // [n, width] each; width 0: no such tensor
    uint32_t width[PLY_GROUPS], first[PLY_GROUPS], act[PLY_GROUPS];
};

uint32_t ply_block_rows(uint32_t stride) {
    for (uint32_t r = 256; r > 64; r >>= 1)
        if (r * stride <= PLY_LDS_BYTES) return r;
    return 64;
}

// the float of one column of the staged row that starts at byte `row`; WORDS: every offset and the stride are multiples of 4
template <bool WORDS> GS_DEV float ply_read(const uint32_t *s_w, uint32_t row, uint32_t col) {
    const uint32_t at = row + (col & PLY_OFFSET_MASK);
    uint32_t lo, hi = 0;
    if (WORDS) {
        lo = s_w[at >> 2];
        if (col & PLY_DOUBLE) hi = s_w[(at >> 2) + 1];
    } else {
        const uint8_t *b = (const uint8_t *)s_w + at;
        lo = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
        if (col & PLY_DOUBLE) hi = (uint32_t)b[4] | ((uint32_t)b[5] << 8) | ((uint32_t)b[6] << 16) | ((uint32_t)b[7] << 24);
    }
    // float64 -> float32 rounds to nearest even, like numpy's astype
    return (col & PLY_DOUBLE) ? (float)__hiloint2double((int)hi, (int)lo) : __uint_as_float(lo);
}

// bytes [0, bytes) of a 16-byte aligned global run <-> the LDS: 16-byte accesses, the last bytes % 16 one by one (nothing
// past the run is touched)
GS_DEV void ply_stage_in(uint4 *s_v, const uint8_t *__restrict__ src, uint32_t bytes) {
    const uint32_t nvec = bytes >> 4;
    for (uint32_t v = threadIdx.x; v < nvec; v += GS_BLOCK) s_v[v] = ((const uint4 *)src)[v];
    for (uint32_t b = (nvec << 4) + threadIdx.x; b < bytes; b += GS_BLOCK) ((uint8_t *)s_v)[b] = src[b];
}
GS_DEV void ply_stage_out(const uint4 *s_v, uint8_t *__restrict__ dst, uint32_t bytes) {
    const uint32_t nvec = bytes >> 4;
    for (uint32_t v = threadIdx.x; v < nvec; v += GS_BLOCK) ((uint4 *)dst)[v] = s_v[v];
    for (uint32_t b = (nvec << 4) + threadIdx.x; b < bytes; b += GS_BLOCK) dst[b] = ((const uint8_t *)s_v)[b];
}

template <bool WORDS>
__global__ void __launch_bounds__(GS_BLOCK) ply_unpack_kernel(uint32_t n, uint32_t stride, uint32_t R, const uint8_t *__restrict__ rows,
                                                              PlyTable t) {
    __shared__ uint4 s_v[PLY_LDS_BYTES / 16];
    const uint32_t *s_w = (const uint32_t *)s_v;
    const uint32_t row0 = blockIdx.x * R; // < n
    const uint32_t count = n - row0 < R ? n - row0 : R;
    ply_stage_in(s_v, rows + (uint64_t)row0 * stride, count * stride); // count * stride <= R * stride <= 64 KB
    __syncthreads();
#pragma unroll
    for (uint32_t g = 0; g < PLY_GROUPS; ++g) {
        const uint32_t W = t.width[g], first = t.first[g], act = t.act[g];
        if (W == 0) continue;
        float *__restrict__ out = t.ptr[g] + (uint64_t)row0 * W;
        if (act == PLY_ACT_NORMALIZE) { // the one place where the elements of a row meet: a lane per row
            for (uint32_t r = threadIdx.x; r < count; r += GS_BLOCK) {
                float acc = 0.f;
                for (uint32_t j = 0; j < W; ++j) {
                    const float q = ply_read<WORDS>(s_w, r * stride, t.col[first + j]);
                    acc = j == 0 ? q * q : decode_sumsq(acc, q);
                }
                const float nrm = decode_norm_divisor(acc);
                for (uint32_t j = 0; j < W; ++j) out[r * W + j] = ply_read<WORDS>(s_w, r * stride, t.col[first + j]) / nrm;
            }
            continue;
        }
        const uint32_t total = count * W; // <= 256 * 128
        for (uint32_t e = threadIdx.x; e < total; e += GS_BLOCK) {
            const uint32_t r = e / W, j = e - r * W;
            const float v = ply_read<WORDS>(s_w, r * stride, t.col[first + j]);
            out[e] = act == PLY_ACT_EXP ? decode_act_scale(v) : (act == PLY_ACT_SIGMOID ? decode_act_opacity(v) : v);
        }
    }
}

// the inverse (float columns at offsets that are multiples of 4, a stride that is one): zeros, the tensors' words, the rows
__global__ void __launch_bounds__(GS_BLOCK) ply_pack_kernel(uint32_t n, uint32_t stride, uint32_t R, PlyTable t, uint8_t *__restrict__ rows) {
    __shared__ uint4 s_v[PLY_LDS_BYTES / 16];
    uint32_t *s_w = (uint32_t *)s_v;
    const uint32_t row0 = blockIdx.x * R;
    const uint32_t count = n - row0 < R ? n - row0 : R;
    const uint32_t bytes = count * stride;
    for (uint32_t v = threadIdx.x; v < (bytes + 15u) >> 4; v += GS_BLOCK) s_v[v] = make_uint4(0u, 0u, 0u, 0u); // (<= 64 KB)
    __syncthreads();
#pragma unroll
    for (uint32_t g = 0; g < PLY_GROUPS; ++g) {
        const uint32_t W = t.width[g], first = t.first[g];
        if (W == 0) continue;
        const float *__restrict__ in = t.ptr[g] + (uint64_t)row0 * W;
        const uint32_t total = count * W;
        for (uint32_t e = threadIdx.x; e < total; e += GS_BLOCK) {
            const uint32_t r = e / W, j = e - r * W;
            s_w[(r * stride + (t.col[first + j] & PLY_OFFSET_MASK)) >> 2] = __float_as_uint(in[e]);
        }
    }
    __syncthreads();
    ply_stage_out(s_v, rows + (uint64_t)row0 * stride, bytes);
}

// The checks both entry points share, and the table by value.  cols / widths6 / ptrs6 are HOST arrays.
int32_t ply_table(const char *who, uint32_t n, uint32_t stride, const void *rows, const uint32_t *cols, const uint32_t *widths6,
                  float *const *ptrs6, bool floats_only, PlyTable *t, bool *words) {
    if (!(n >= 1 && n < (1u << 31))) { gs_set_error("%s: need 1 <= n < 2^31", who); return 1; }
    if (!(rows && cols && widths6 && ptrs6)) { gs_set_error("%s: null pointer", who); return 1; }
    if (!(stride >= 1 && stride <= PLY_MAX_STRIDE)) { gs_set_error("%s: need 1 <= stride <= %u bytes", who, PLY_MAX_STRIDE); return 1; }
    if ((uintptr_t)rows % 16u != 0) { gs_set_error("%s: the rows must be 16-byte aligned", who); return 1; }
    uint32_t total = 0;
    *words = stride % 4u == 0;
    for (uint32_t g = 0; g < PLY_GROUPS; ++g) {
        if (widths6[g] > PLY_MAX_COLUMNS || total + widths6[g] > PLY_MAX_COLUMNS) {
            gs_set_error("%s: more than %u columns", who, PLY_MAX_COLUMNS);
            return 1;
        }
        if (widths6[g] != 0 && ptrs6[g] == nullptr) { gs_set_error("%s: null pointer (tensor %u)", who, g); return 1; }
        t->width[g] = widths6[g], t->first[g] = total, t->ptr[g] = ptrs6[g], t->act[g] = PLY_ACT_NONE;
        total += widths6[g];
    }
    if (total == 0) { gs_set_error("%s: no columns", who); return 1; }
    for (uint32_t c = 0; c < PLY_MAX_COLUMNS; ++c) {
        const uint32_t col = c < total ? cols[c] : 0u;
        const uint32_t off = col & PLY_OFFSET_MASK, size = (col & PLY_DOUBLE) ? 8u : 4u;
        if ((col & ~(PLY_OFFSET_MASK | PLY_DOUBLE)) != 0 || (floats_only && (col & PLY_DOUBLE))) {
            gs_set_error("%s: column %u: unknown type flag", who, c);
            return 1;
        }
        if (c < total && off + size > stride) { gs_set_error("%s: column %u: offset %u beyond the stride %u", who, c, off, stride); return 1; }
        if (off % 4u != 0) *words = false;
        t->col[c] = col;
    }
    return 0;
}

} // namespace

extern "C" uint32_t gs_ply_max_stride(void) { return PLY_MAX_STRIDE; }
extern "C" uint32_t gs_ply_max_columns(void) { return PLY_MAX_COLUMNS; }
extern "C" uint32_t gs_ply_block_rows(uint32_t stride) { return stride >= 1 && stride <= PLY_MAX_STRIDE ? ply_block_rows(stride) : 0; }

extern "C" int32_t gs_ply_unpack(uint32_t n, uint32_t stride, const uint8_t *rows, const uint32_t *cols, const uint32_t *widths6,
                                 float *const *outs6, int32_t activate, int32_t normalize_quats, int32_t force_bytes, gs_stream_t stream) {
    PlyTable t;
    bool words;
    if (ply_table(__func__, n, stride, rows, cols, widths6, outs6, false, &t, &words)) return 1;
    if (activate) t.act[3] = PLY_ACT_SIGMOID, t.act[4] = PLY_ACT_EXP;
    if (normalize_quats) t.act[5] = PLY_ACT_NORMALIZE;
    const uint32_t R = ply_block_rows(stride);
    const dim3 grid(gs_div_up(n, R)), block(GS_BLOCK);
    if (words && !force_bytes) hipLaunchKernelGGL(ply_unpack_kernel<true>, grid, block, 0, (hipStream_t)stream, n, stride, R, rows, t);
    else hipLaunchKernelGGL(ply_unpack_kernel<false>, grid, block, 0, (hipStream_t)stream, n, stride, R, rows, t);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_ply_pack(uint32_t n, uint32_t stride, const uint32_t *cols, const uint32_t *widths6, const float *const *ins6,
                               uint8_t *rows, gs_stream_t stream) {
    PlyTable t;
    bool words;
    if (ply_table(__func__, n, stride, rows, cols, widths6, (float *const *)ins6, true, &t, &words)) return 1;
    GS_CHECK_ARG(words, "the stride and every offset must be multiples of 4");
    const uint32_t R = ply_block_rows(stride);
    hipLaunchKernelGGL(ply_pack_kernel, dim3(gs_div_up(n, R)), dim3(GS_BLOCK), 0, (hipStream_t)stream, n, stride, R, t, rows);
    GS_CHECK_LAUNCH();
    return 0;
}
