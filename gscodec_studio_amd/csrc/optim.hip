// optim.hip -- Adam and SelectiveAdam over several tensors in one launch (gs_adam_multi), and SparseAdam over several tensors
// that share one index list (gs_sparse_adam_multi, second half of the file).
//
// Dense mode: torch.optim.adam._single_tensor_adam (non-capturable) per element, in its order of operations:
//   m = lerp(m, g, 1 - b1)            (ATen's two-branch lerp)
//   v = v * b2;  v = v + ((1 - b2) * g) * g
//   denom = sqrt(v) / bc2_sqrt + eps
//   p = p + (-step_size) * (m / denom)
// with step_size = lr / (1 - b1^step) and bc2_sqrt = (1 - b2^step)^0.5 computed by the host in double, as torch does.
// Selective mode: gsplat/cuda/csrc/adam.cu:31-40 as written (no bias correction), only where visibility[e / M] is set; the
// elements of the other rows are neither read nor written.
//
// Layout: every descriptor of a launch is cut into chunks of GS_BLOCK * ADAM_UNROLL quads (4 floats), and the chunks of all the
// tensors form one index space (prefix sums in the kernel arguments) that a device-sized grid strides over, so a 45 M-float shN
// and a 1 M-float opacity vector cost the same per chunk.  Within a tensor, quads start behind a head of 0-3 elements that brings
// the four pointers to a 16-B boundary (when they share their offset mod 16; otherwise every element goes scalar).  No atomics:
// every element is written by one thread, and the results do not depend on the grid.
// Compiled with -ffp-contract=off (Makefile STRICT): the arithmetic above rounds after every operation, as torch's kernels do.
#include "gs_common.h"

#define ADAM_UNROLL 1
#define ADAM_CHUNK_QUADS (GS_BLOCK * ADAM_UNROLL)

namespace {

struct AdamTensor {
    float *p;
    const float *g;
    float *m, *v;
    const uint8_t *vis;  // selective: [rows]
    uint64_t n;          // floats
    uint32_t head;       // elements ahead of the first 16-B aligned quad (vec) -- all scalar
    uint32_t vec;        // p, g, m, v share their offset mod 16
    uint32_t magic, sh1, sh2;  // e / row_width = (t + ((e - t) >> sh1)) >> sh2, t = umulhi(e, magic)
    uint32_t mode;
    // dense: c0 = 1 - b1 (lerp weight), c1 = b2, c2 = 1 - b2, c3 = -step_size, c4 = bc2_sqrt, c5 = eps
    // selective: c0 = b1, c1 = b2, c2 = 1 - b2, c3 = -lr, c4 = 1 - b1, c5 = eps
    float c0, c1, c2, c3, c4, c5;
};

struct AdamMultiArgs {
    uint32_t n;
    uint32_t chunk_end[GS_ADAM_MULTI_MAX];  // inclusive prefix sum of the tensors' chunk counts
    AdamTensor t[GS_ADAM_MULTI_MAX];
};

GS_DEV void adam_dense(float &p, float g, float &m, float &v, const AdamTensor &d) {
    GS_FP_STRICT
    const float w = d.c0;
    m = fabsf(w) < 0.5f ? m + w * (g - m) : g - (g - m) * (1.f - w);
    v = v * d.c1;
    v = v + (d.c2 * g) * g;
    const float denom = sqrtf(v) / d.c4 + d.c5;
    p = p + d.c3 * (m / denom);
}

GS_DEV void adam_selective(float &p, float g, float &m, float &v, const AdamTensor &d) {
    GS_FP_STRICT
    m = d.c0 * m + d.c4 * g;
    v = d.c1 * v + (d.c2 * g) * g;
    p = p + (d.c3 * m) / (sqrtf(v) + d.c5);
}

template <bool SEL>
GS_DEV void adam_one(float &p, float g, float &m, float &v, const AdamTensor &d) {
    if (SEL) adam_selective(p, g, m, v, d);
    else adam_dense(p, g, m, v, d);
}

GS_DEV uint32_t row_of(uint32_t e, const AdamTensor &d) {
    const uint32_t t = __umulhi(e, d.magic);
    return (t + ((e - t) >> d.sh1)) >> d.sh2;
}

template <bool SEL>
GS_DEV bool visible(uint64_t e, const AdamTensor &d) {
    return !SEL || d.vis[row_of((uint32_t)e, d)] != 0;
}

template <bool SEL>
GS_DEV void adam_scalar(uint64_t e, const AdamTensor &d) {
    if (!visible<SEL>(e, d)) return;
    float p = d.p[e], m = d.m[e], v = d.v[e];
    adam_one<SEL>(p, d.g[e], m, v, d);
    d.p[e] = p;
    d.m[e] = m;
    d.v[e] = v;
}

// one chunk of one tensor: ADAM_UNROLL quads per thread, lane-contiguous (quad q0 + k * GS_BLOCK + threadIdx.x)
template <bool SEL>
GS_DEV void adam_chunk(const AdamTensor &d, uint64_t q0, bool first) {
    const uint32_t tid = threadIdx.x;
    if (first && tid < d.head) adam_scalar<SEL>(tid, d);
    uint64_t e[ADAM_UNROLL];
    // 0: nothing, 1: whole quad as 16-B accesses, 2: element by element (tail, misaligned tensor, mixed visibility)
    uint32_t how[ADAM_UNROLL];
    float4 P[ADAM_UNROLL], G[ADAM_UNROLL], M[ADAM_UNROLL], V[ADAM_UNROLL];
#pragma unroll
    for (int k = 0; k < ADAM_UNROLL; ++k) {
        e[k] = d.head + 4ull * (q0 + (uint64_t)k * GS_BLOCK + tid);
        how[k] = e[k] >= d.n ? 0u : (d.vec && e[k] + 4 <= d.n) ? 1u : 2u;
        if (SEL && how[k] == 1u) {
            const uint32_t r0 = row_of((uint32_t)e[k], d), r3 = row_of((uint32_t)e[k] + 3u, d);
            if (r0 == r3) {
                how[k] = d.vis[r0] ? 1u : 0u;
            } else {
                const uint32_t nv = (d.vis[r0] != 0) + (d.vis[row_of((uint32_t)e[k] + 1u, d)] != 0) +
                                    (d.vis[row_of((uint32_t)e[k] + 2u, d)] != 0) + (d.vis[r3] != 0);
                how[k] = nv == 4u ? 1u : nv == 0u ? 0u : 2u;
            }
        }
        if (how[k] == 1u) {
            P[k] = *reinterpret_cast<const float4 *>(d.p + e[k]);
            G[k] = *reinterpret_cast<const float4 *>(d.g + e[k]);
            M[k] = *reinterpret_cast<const float4 *>(d.m + e[k]);
            V[k] = *reinterpret_cast<const float4 *>(d.v + e[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < ADAM_UNROLL; ++k) {
        if (how[k] == 1u) {
            adam_one<SEL>(P[k].x, G[k].x, M[k].x, V[k].x, d);
            adam_one<SEL>(P[k].y, G[k].y, M[k].y, V[k].y, d);
            adam_one<SEL>(P[k].z, G[k].z, M[k].z, V[k].z, d);
            adam_one<SEL>(P[k].w, G[k].w, M[k].w, V[k].w, d);
            *reinterpret_cast<float4 *>(d.p + e[k]) = P[k];
            *reinterpret_cast<float4 *>(d.m + e[k]) = M[k];
            *reinterpret_cast<float4 *>(d.v + e[k]) = V[k];
        } else if (how[k] == 2u) {
            const uint64_t end = e[k] + 4 < d.n ? e[k] + 4 : d.n;
            for (uint64_t i = e[k]; i < end; ++i) adam_scalar<SEL>(i, d);
        }
    }
}

__global__ void __launch_bounds__(GS_BLOCK) adam_multi_kernel(AdamMultiArgs a) {
    const uint32_t total = a.chunk_end[a.n - 1];
    uint32_t t = 0;
    // chunks ascend along the grid stride, so the tensor index only moves forward (block-uniform)
    for (uint32_t c = blockIdx.x; c < total; c += gridDim.x) {
        while (c >= a.chunk_end[t]) ++t;
        const uint32_t c0 = t ? a.chunk_end[t - 1] : 0u;
        const AdamTensor &d = a.t[t];
        const uint64_t q0 = (uint64_t)(c - c0) * ADAM_CHUNK_QUADS;
        if (d.mode == GS_ADAM_SELECTIVE) adam_chunk<true>(d, q0, c == c0);
        else adam_chunk<false>(d, q0, c == c0);
    }
}

// the device's resident-block budget: CUs x (max threads per CU / GS_BLOCK), what torch sizes its stream kernels by
int32_t device_grid_cap(uint32_t *cap) {
    static uint32_t cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 1;
    if (dev < 64 && cache[dev]) {
        *cap = cache[dev];
        return 0;
    }
    int cus = 0, thr = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipDeviceGetAttribute(&thr, hipDeviceAttributeMaxThreadsPerMultiProcessor, dev) != hipSuccess || cus <= 0 || thr < GS_BLOCK)
        return 1;
    *cap = (uint32_t)cus * (uint32_t)(thr / GS_BLOCK);
    if (dev < 64) cache[dev] = *cap;
    return 0;
}

// Granlund-Montgomery round-up division by an invariant divisor, exact for every 32-bit dividend
void div_magic(uint32_t dv, uint32_t &magic, uint32_t &sh1, uint32_t &sh2) {
    uint32_t l = 0;
    while (l < 32 && (1ull << l) < dv) ++l;
    magic = (uint32_t)(((1ull << 32) * ((1ull << l) - dv)) / dv + 1);
    sh1 = l < 1 ? l : 1u;
    sh2 = l > 0 ? l - 1 : 0u;
}

// ---------------------------------------------------------------------------------------------------------------------------
// SparseAdam (gs_sparse_adam_multi): torch.optim._functional.sparse_adam per element of the rows that have a gradient, in its
// order of operations (every line one float32 rounding):
//   g  = the sum of the duplicates' values
//   d1 = (g - m) * w1            d2 = (g * g - v) * w2
//   m' = m + d1                  v' = v + d2
//   p' = p + s * ((d1 + m) / (sqrt(d2 + v) + eps))
// with w1 = 1 - beta1, w2 = 1 - beta2 and s = -(lr * sqrt(1 - beta2^step) / (1 - beta1^step)) computed by the host in double and
// rounded to float.  Rows without an index are neither read nor written.
//
// Mapping: one lane per (sorted position k, column c), element e = k * row_width + c (k by the magic division above), so the
// lanes of a row are contiguous in values, p, m and v alike.  sorted_ids ascends; a lane whose id equals its predecessor's is not
// the head of its run and returns.  A head lane walks forward over its run and adds values[perm[j] * row_width + c] in the order
// of j: the sort behind sorted_ids / perm is stable on (id, position), so a run is summed in ascending position in values,
// starting from its first value -- THE defined order of the duplicates' sum (torch's own coalesce() uses another for three or
// more).  A run of length r costs r serial loads per column; the trainers produce r <= the number of cameras, so there is no
// second path for long runs.  Every (row, column) is written by exactly one lane: no atomics, results bit-identical from run to
// run and independent of the grid.  Chunks (GS_BLOCK elements) of all the tensors form one index space that a device-sized grid
// strides over, as above.  An id outside [0, rows) or a perm entry outside [0, nnz) is skipped, never used as an address.
struct SparseAdamTensor {
    float *p, *m, *v;
    const float *g;            // values [nnz, row_width]
    uint32_t row_width, n;     // n = nnz * row_width elements
    uint32_t magic, sh1, sh2;  // e / row_width, as in AdamTensor
    float w1, w2, s, eps;
};

struct SparseAdamMultiArgs {
    uint32_t n;
    uint32_t nnz;
    uint64_t rows;
    const int64_t *ids;   // [nnz] ascending
    const int32_t *perm;  // [nnz] or null (identity)
    uint32_t chunk_end[GS_ADAM_MULTI_MAX];
    SparseAdamTensor t[GS_ADAM_MULTI_MAX];
};

GS_DEV void sparse_adam_one(float &p, float g, float &m, float &v, const SparseAdamTensor &d) {
    GS_FP_STRICT
    const float d1 = (g - m) * d.w1;
    const float d2 = (g * g - v) * d.w2;
    const float numer = d1 + m;
    const float denom = sqrtf(d2 + v) + d.eps;
    m = m + d1;
    v = v + d2;
    p = p + d.s * (numer / denom);
}

__global__ void __launch_bounds__(GS_BLOCK) sparse_adam_multi_kernel(SparseAdamMultiArgs a) {
    const uint32_t total = a.chunk_end[a.n - 1];
    uint32_t t = 0;
    for (uint32_t ch = blockIdx.x; ch < total; ch += gridDim.x) {
        while (ch >= a.chunk_end[t]) ++t;
        const uint32_t c0 = t ? a.chunk_end[t - 1] : 0u;
        const SparseAdamTensor &d = a.t[t];
        const uint64_t e64 = (uint64_t)(ch - c0) * GS_BLOCK + threadIdx.x;
        if (e64 >= d.n) continue;
        const uint32_t e = (uint32_t)e64;
        const uint32_t tq = __umulhi(e, d.magic);
        const uint32_t k = (tq + ((e - tq) >> d.sh1)) >> d.sh2;
        const uint32_t c = e - k * d.row_width;
        const int64_t id = a.ids[k];
        if (k > 0 && a.ids[k - 1] == id) continue;      // not the head of its run
        if (id < 0 || (uint64_t)id >= a.rows) continue;  // never an address
        float g = 0.f;
        bool first = true;
        for (uint32_t j = k; j < a.nnz && a.ids[j] == id; ++j) {
            const uint32_t src = a.perm ? (uint32_t)a.perm[j] : j;
            if (src >= a.nnz) continue;
            const float x = d.g[(uint64_t)src * d.row_width + c];
            g = first ? x : g + x;  // (starts from the first value: -0 stays -0)
            first = false;
        }
        if (first) continue;
        const uint64_t o = (uint64_t)id * d.row_width + c;
        float p = d.p[o], m = d.m[o], v = d.v[o];
        sparse_adam_one(p, g, m, v, d);
        d.p[o] = p;
        d.m[o] = m;
        d.v[o] = v;
    }
}

}  // namespace

extern "C" uint32_t gs_adam_multi_max(void) { return GS_ADAM_MULTI_MAX; }

extern "C" uint32_t gs_adam_desc_layout(uint64_t *out, uint32_t n) {
    const uint64_t v[] = {sizeof(gs_adam_desc), offsetof(gs_adam_desc, n), offsetof(gs_adam_desc, param), offsetof(gs_adam_desc, grad),
                          offsetof(gs_adam_desc, exp_avg), offsetof(gs_adam_desc, exp_avg_sq), offsetof(gs_adam_desc, visibility),
                          offsetof(gs_adam_desc, rows), offsetof(gs_adam_desc, row_width), offsetof(gs_adam_desc, lr),
                          offsetof(gs_adam_desc, step_size), offsetof(gs_adam_desc, mode)};
    const uint32_t m = (uint32_t)(sizeof(v) / sizeof(v[0]));
    for (uint32_t i = 0; out != nullptr && i < n && i < m; ++i) out[i] = v[i];
    return m;
}

extern "C" int32_t gs_adam_multi(uint32_t n_tensors, const gs_adam_desc *descs, gs_stream_t stream) {
    GS_CHECK_ARG(n_tensors == 0 || descs != nullptr, "null descriptor table");
    // every descriptor is checked before anything is launched: a bad one leaves all the tensors untouched
    for (uint32_t i = 0; i < n_tensors; ++i) {
        const gs_adam_desc &d = descs[i];
        if (d.n == 0) continue;
        if (!d.param || !d.grad || !d.exp_avg || !d.exp_avg_sq) {
            gs_set_error("gs_adam_multi: descriptor %u: null pointer", i);
            return 1;
        }
        if (d.mode != GS_ADAM_DENSE && d.mode != GS_ADAM_SELECTIVE) {
            gs_set_error("gs_adam_multi: descriptor %u: unknown mode %d", i, d.mode);
            return 1;
        }
        if (((uintptr_t)d.param | (uintptr_t)d.grad | (uintptr_t)d.exp_avg | (uintptr_t)d.exp_avg_sq) % 4 != 0) {
            gs_set_error("gs_adam_multi: descriptor %u: float arrays must be 4-byte aligned", i);
            return 1;
        }
        if (d.mode == GS_ADAM_SELECTIVE &&
            (!d.visibility || d.rows == 0 || d.row_width == 0 || d.row_width >= (1u << 31) || (uint64_t)d.rows * d.row_width != d.n ||
             d.n > 0xffffffffull)) {
            gs_set_error("gs_adam_multi: descriptor %u: selective mode needs visibility[rows], n = rows * row_width < 2^32, row_width < 2^31", i);
            return 1;
        }
    }
    uint32_t cap = 0;
    if (device_grid_cap(&cap)) {
        gs_set_error("gs_adam_multi: cannot query the current device");
        return 1;
    }
    const hipStream_t st = (hipStream_t)stream;
    AdamMultiArgs a;
    uint64_t chunks = 0;
    a.n = 0;
    for (uint32_t i = 0; i <= n_tensors; ++i) {
        // launch when the table is full or the descriptors are used up
        if (a.n == GS_ADAM_MULTI_MAX || (i == n_tensors && a.n > 0)) {
            if (chunks > 0xffffffffull) {
                gs_set_error("gs_adam_multi: more than 2^32 chunks in one launch");
                return 1;
            }
            const uint32_t blocks = chunks < cap ? (uint32_t)chunks : cap;
            hipLaunchKernelGGL(adam_multi_kernel, dim3(blocks), dim3(GS_BLOCK), 0, st, a);
            GS_CHECK_LAUNCH();
            a.n = 0;
            chunks = 0;
        }
        if (i == n_tensors) break;
        const gs_adam_desc &d = descs[i];
        if (d.n == 0) continue;
        AdamTensor &t = a.t[a.n];
        t.p = d.param;
        t.g = d.grad;
        t.m = d.exp_avg;
        t.v = d.exp_avg_sq;
        t.vis = d.visibility;
        t.n = d.n;
        const uintptr_t off = (uintptr_t)d.param % 16;
        t.vec = (off == (uintptr_t)d.grad % 16 && off == (uintptr_t)d.exp_avg % 16 && off == (uintptr_t)d.exp_avg_sq % 16) ? 1u : 0u;
        t.head = t.vec ? (uint32_t)((16 - off) % 16 / 4) : 0u;
        if (t.head > d.n) t.head = (uint32_t)d.n;
        t.mode = (uint32_t)d.mode;
        t.magic = 1u;
        t.sh1 = t.sh2 = 0u;
        if (d.mode == GS_ADAM_SELECTIVE) {
            div_magic(d.row_width, t.magic, t.sh1, t.sh2);
            t.c0 = d.beta1;
            t.c1 = d.beta2;
            t.c2 = 1.0f - d.beta2;
            t.c3 = -d.lr;
            t.c4 = 1.0f - d.beta1;
        } else {
            t.c0 = d.one_minus_beta1;
            t.c1 = d.beta2;
            t.c2 = d.one_minus_beta2;
            t.c3 = -d.step_size;
            t.c4 = d.bias_correction2_sqrt;
        }
        t.c5 = d.eps;
        const uint64_t quads = (d.n - t.head + 3) / 4;
        uint64_t c = (quads + ADAM_CHUNK_QUADS - 1) / ADAM_CHUNK_QUADS;
        if (c == 0) c = 1;  // a tensor that is all head
        chunks += c;
        a.chunk_end[a.n] = (uint32_t)(chunks < 0xffffffffull ? chunks : 0xffffffffull);
        ++a.n;
    }
    return 0;
}

extern "C" uint32_t gs_sparse_adam_desc_layout(uint64_t *out, uint32_t n) {
    const uint64_t v[] = {sizeof(gs_sparse_adam_desc), offsetof(gs_sparse_adam_desc, param), offsetof(gs_sparse_adam_desc, exp_avg),
                          offsetof(gs_sparse_adam_desc, exp_avg_sq), offsetof(gs_sparse_adam_desc, values),
                          offsetof(gs_sparse_adam_desc, row_width), offsetof(gs_sparse_adam_desc, one_minus_beta1),
                          offsetof(gs_sparse_adam_desc, one_minus_beta2), offsetof(gs_sparse_adam_desc, neg_step_size),
                          offsetof(gs_sparse_adam_desc, eps)};
    const uint32_t m = (uint32_t)(sizeof(v) / sizeof(v[0]));
    for (uint32_t i = 0; out != nullptr && i < n && i < m; ++i) out[i] = v[i];
    return m;
}

extern "C" int32_t gs_sparse_adam_multi(uint32_t n_tensors, const gs_sparse_adam_desc *descs, uint64_t nnz, const int64_t *sorted_ids,
                                        const int32_t *perm, uint64_t rows, gs_stream_t stream) {
    GS_CHECK_ARG(n_tensors == 0 || descs != nullptr, "null descriptor table");
    GS_CHECK_ARG(nnz < (1ull << 31), "nnz must be < 2^31");
    if (nnz == 0 || n_tensors == 0) return 0;
    GS_CHECK_ARG(sorted_ids != nullptr, "null sorted_ids");
    GS_CHECK_ARG((uintptr_t)sorted_ids % 8 == 0 && (uintptr_t)perm % 4 == 0, "sorted_ids must be 8-byte, perm 4-byte aligned");
    // every descriptor is checked before anything is launched: a bad one leaves all the tensors untouched
    for (uint32_t i = 0; i < n_tensors; ++i) {
        const gs_sparse_adam_desc &d = descs[i];
        if (!d.param || !d.exp_avg || !d.exp_avg_sq || !d.values) {
            gs_set_error("gs_sparse_adam_multi: descriptor %u: null pointer", i);
            return 1;
        }
        if (((uintptr_t)d.param | (uintptr_t)d.exp_avg | (uintptr_t)d.exp_avg_sq | (uintptr_t)d.values) % 4 != 0) {
            gs_set_error("gs_sparse_adam_multi: descriptor %u: float arrays must be 4-byte aligned", i);
            return 1;
        }
        if (d.row_width == 0 || d.row_width >= (1u << 31) || nnz * d.row_width > 0xffffffffull || rows > 0xffffffffull ||
            rows * d.row_width > 0xffffffffull) {
            gs_set_error("gs_sparse_adam_multi: descriptor %u: needs 1 <= row_width < 2^31, nnz * row_width < 2^32 and "
                         "rows * row_width < 2^32", i);
            return 1;
        }
    }
    uint32_t cap = 0;
    if (device_grid_cap(&cap)) {
        gs_set_error("gs_sparse_adam_multi: cannot query the current device");
        return 1;
    }
    const hipStream_t st = (hipStream_t)stream;
    SparseAdamMultiArgs a;
    a.nnz = (uint32_t)nnz;
    a.rows = rows;
    a.ids = sorted_ids;
    a.perm = perm;
    for (uint32_t i0 = 0; i0 < n_tensors; i0 += GS_ADAM_MULTI_MAX) {
        a.n = n_tensors - i0 < GS_ADAM_MULTI_MAX ? n_tensors - i0 : GS_ADAM_MULTI_MAX;
        uint32_t chunks = 0;  // (16 tensors of < 2^24 chunks each)
        for (uint32_t i = 0; i < a.n; ++i) {
            const gs_sparse_adam_desc &d = descs[i0 + i];
            SparseAdamTensor &t = a.t[i];
            t.p = d.param;
            t.m = d.exp_avg;
            t.v = d.exp_avg_sq;
            t.g = d.values;
            t.row_width = d.row_width;
            t.n = (uint32_t)(nnz * d.row_width);
            div_magic(d.row_width, t.magic, t.sh1, t.sh2);
            t.w1 = d.one_minus_beta1;
            t.w2 = d.one_minus_beta2;
            t.s = d.neg_step_size;
            t.eps = d.eps;
            chunks += (uint32_t)(((uint64_t)t.n + GS_BLOCK - 1) / GS_BLOCK);
            a.chunk_end[i] = chunks;
        }
        const uint32_t blocks = chunks < cap ? chunks : cap;
        hipLaunchKernelGGL(sparse_adam_multi_kernel, dim3(blocks), dim3(GS_BLOCK), 0, st, a);
        GS_CHECK_LAUNCH();
    }
    return 0;
}
