// kmeans.hip -- the Lloyd steps of the shN codebook in fixed point: manhattan assignment and mean update (gfx950).
//
// The reference clusters the higher SH bands with `torchpq`'s K-means (gsplat/compression/png_compression.py:420-484); here the
// algorithm is the library's own, defined by the numpy code gscodec_studio_amd/compression/kmeans_reference.py, and every
// kernel below is integer arithmetic whose result equals it element for element, whatever the tiling or the order of the adds:
//
//   gs_kmeans_assign   label[i] = the lowest j with the least d(i, j) = sum over the channels of |q[i, c] - cent[j, c]|
//   gs_kmeans_update   cent[j, c] = (2 s + cnt) / (2 cnt) over the members of cluster j (an empty cluster keeps its centroid)
//
// Assign: the points are channel-major [w, n], so a lane loads its point's words coalesced and keeps them in registers, the
// width padded to one of KMEANS_WIDTHS (padded channels are zero in the point and in the centroid rows, which are [k, wp]).  A
// lane owns two points (one at the widest width) and walks a slice of the centroids; a centroid row is wave-uniform, so it
// arrives in SGPRs through scalar loads and every (point, centroid, channel) costs one v_sad_u32 with the SGPR as its second
// source.  d <= 64 * (2^24 - 1) < 2^30.  With one slice the lane writes its label; with several (few points, many centroids:
// n / 512 workgroups would leave the CUs idle) the slices meet in a 64-bit unsigned minimum over d << 32 | j, which is the
// least distance and on ties the lowest index in any arrival order, and a second kernel takes the labels out of the keys.
//
// Update: zero-fill, then one lane per (channel, point) element adds into sums[k, w] (64-bit integer atomics) and the lanes of
// channel 0 into counts[k]; then one lane per (cluster, channel) divides.  Integer atomics: the sums do not depend on the order.
#include "gs_common.h"

namespace {

constexpr uint32_t KMEANS_MAX_W = 64;
constexpr uint32_t KMEANS_MAX_K = 1u << 20;
constexpr uint32_t KMEANS_WIDTHS[] = {4, 8, 16, 32, 48, 64};

uint32_t kmeans_padded_width(uint32_t w) {
    if (w < 1 || w > KMEANS_MAX_W) return 0;
    for (uint32_t wp : KMEANS_WIDTHS)
        if (w <= wp) return wp;
    return 0;
}

// points per lane at a padded width: two rows of 48 words still leave four waves per SIMD, two of 64 would not
constexpr uint32_t kmeans_points_per_lane(uint32_t wp) { return wp <= 48 ? 2u : 1u; }

typedef uint32_t kmeans_u32x4 __attribute__((ext_vector_type(4)));

// acc + |a[0] - b.x| + ... + |a[3] - b.w|, one v_sad_u32 per term; `b` is wave-uniform (four words of a centroid row held in
// SGPRs, the instruction's second source).  __usad() lowers to v_max_u32 + v_min_u32 and a share of a v_add3_u32 here, about
// three instructions per term.  One statement per quad: the compiler pads every asm statement's result with a wait state, the
// dependent instructions inside need none.
GS_DEV uint32_t sad4_u32(const uint32_t *a, kmeans_u32x4 b, uint32_t acc) {
    asm("v_sad_u32 %0, %1, %5, %0\n\tv_sad_u32 %0, %2, %6, %0\n\tv_sad_u32 %0, %3, %7, %0\n\tv_sad_u32 %0, %4, %8, %0"
        : "+v"(acc)
        : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "s"(b.x), "s"(b.y), "s"(b.z), "s"(b.w));
    return acc;
}

// SLICED: blockIdx.y owns the centroids [blockIdx.y * slice_len, + slice_len) and the result goes into keys[] by atomic minimum;
// otherwise the one slice is all of them and the lane writes its labels and counts the changed ones.
template <uint32_t WP, uint32_t P, bool SLICED>
__global__ void __launch_bounds__(GS_BLOCK) kmeans_assign_kernel(uint32_t n, uint32_t w, uint32_t k, uint32_t slice_len,
                                                                 const uint32_t *__restrict__ q, const uint32_t *__restrict__ cent,
                                                                 unsigned long long *__restrict__ keys, int32_t *__restrict__ labels,
                                                                 uint32_t *__restrict__ n_changed) {
    const uint64_t first = ((uint64_t)blockIdx.x * GS_BLOCK + threadIdx.x) * P;
    if (first >= n) return;
    uint32_t x[P][WP];
#pragma unroll
    for (uint32_t p = 0; p < P; ++p) {
        const uint64_t i = first + p < n ? first + p : first; // the second point of the last lane: a copy, never written
#pragma unroll
        for (uint32_t c = 0; c < WP; ++c) { // a padded channel re-reads the last one and drops it: loads without branches
            const uint32_t v = q[(uint64_t)(c < w ? c : w - 1u) * n + i];
            x[p][c] = c < w ? v : 0u;
        }
    }
    const uint32_t j0 = SLICED ? blockIdx.y * slice_len : 0u;
    const uint32_t j1 = SLICED ? (k - j0 < slice_len ? k : j0 + slice_len) : k;
    uint32_t best_d[P], best_j[P];
#pragma unroll
    for (uint32_t p = 0; p < P; ++p) {
        best_d[p] = 0xFFFFFFFFu;
        best_j[p] = j0;
    }
    for (uint32_t j = j0; j < j1; ++j) {
        const kmeans_u32x4 *row = (const kmeans_u32x4 *)cent + j * (WP / 4u); // k * wp / 4 <= 2^24 quads: 32-bit index arithmetic
        uint32_t d[P];
#pragma unroll
        for (uint32_t p = 0; p < P; ++p) d[p] = 0u;
#pragma unroll
        for (uint32_t c4 = 0; c4 < WP / 4u; ++c4) {
            const kmeans_u32x4 s = row[c4];
#pragma unroll
            for (uint32_t p = 0; p < P; ++p) d[p] = sad4_u32(&x[p][4u * c4], s, d[p]);
        }
#pragma unroll
        for (uint32_t p = 0; p < P; ++p)
            if (d[p] < best_d[p]) { // strict, j ascending: a tie keeps the lower index
                best_d[p] = d[p];
                best_j[p] = j;
            }
    }
#pragma unroll
    for (uint32_t p = 0; p < P; ++p) {
        const uint64_t i = first + p;
        if (i >= n) break;
        if (SLICED) {
            atomicMin(&keys[i], ((unsigned long long)best_d[p] << 32) | best_j[p]);
        } else {
            if (labels[i] != (int32_t)best_j[p]) atomicAdd(n_changed, 1u); // (compiled to one add of the lane count per wave)
            labels[i] = (int32_t)best_j[p];
        }
    }
}

// every key was written by the atomic minimum of the slice kernel after the 0xFF fill: its low word is a centroid index
__global__ void __launch_bounds__(GS_BLOCK) kmeans_labels_kernel(uint32_t n, const unsigned long long *__restrict__ keys,
                                                                 int32_t *__restrict__ labels, uint32_t *__restrict__ n_changed) {
    const uint32_t i = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t label = (int32_t)(uint32_t)keys[i];
    if (labels[i] != label) atomicAdd(n_changed, 1u);
    labels[i] = label;
}

__global__ void __launch_bounds__(GS_BLOCK) kmeans_accumulate_kernel(uint32_t n, uint32_t w, uint32_t k, const uint32_t *__restrict__ q,
                                                                     const int32_t *__restrict__ labels,
                                                                     unsigned long long *__restrict__ sums, uint32_t *__restrict__ counts) {
    const uint64_t e = (uint64_t)blockIdx.x * GS_BLOCK + threadIdx.x;
    if (e >= (uint64_t)n * w) return;
    const uint32_t c = (uint32_t)(e / n);
    const uint32_t i = (uint32_t)(e - (uint64_t)c * n);
    const uint32_t j = (uint32_t)labels[i];
    if (j >= k) return; // a label that is no cluster index adds nowhere
    atomicAdd(&sums[(uint64_t)j * w + c], (unsigned long long)q[e]);
    if (c == 0u) atomicAdd(&counts[j], 1u);
}

__global__ void __launch_bounds__(GS_BLOCK) kmeans_finalise_kernel(uint32_t w, uint32_t wp, uint32_t k,
                                                                   const unsigned long long *__restrict__ sums,
                                                                   const uint32_t *__restrict__ counts, uint32_t *__restrict__ cent) {
    const uint32_t t = blockIdx.x * GS_BLOCK + threadIdx.x; // k * w <= 2^26
    if (t >= k * w) return;
    const uint32_t j = t / w, c = t - j * w;
    const unsigned long long cnt = counts[j];
    if (cnt == 0ull) return;
    cent[(uint64_t)j * wp + c] = (uint32_t)((2ull * sums[t] + cnt) / (2ull * cnt)); // s <= n * (2^24 - 1) < 2^55
}

template <uint32_t WP>
void kmeans_launch_assign(uint32_t n, uint32_t w, uint32_t k, uint32_t k_slices, const uint32_t *q, const uint32_t *cent,
                          unsigned long long *keys, int32_t *labels, uint32_t *n_changed, hipStream_t stream) {
    constexpr uint32_t P = kmeans_points_per_lane(WP);
    const uint32_t blocks = gs_div_up(n, (uint64_t)GS_BLOCK * P);
    if (k_slices == 1u) {
        hipLaunchKernelGGL((kmeans_assign_kernel<WP, P, false>), dim3(blocks), dim3(GS_BLOCK), 0, stream, n, w, k, k, q, cent, keys, labels,
                           n_changed);
        return;
    }
    const uint32_t slice_len = gs_div_up(k, k_slices);
    hipLaunchKernelGGL((kmeans_assign_kernel<WP, P, true>), dim3(blocks, gs_div_up(k, slice_len)), dim3(GS_BLOCK), 0, stream, n, w, k,
                       slice_len, q, cent, keys, labels, n_changed);
    hipLaunchKernelGGL(kmeans_labels_kernel, dim3(gs_div_up(n, GS_BLOCK)), dim3(GS_BLOCK), 0, stream, n, keys, labels, n_changed);
}

bool kmeans_shape_ok(uint32_t n, uint32_t w, uint32_t k) {
    return n >= 1 && n < (1u << 31) && w >= 1 && w <= KMEANS_MAX_W && k >= 1 && k <= KMEANS_MAX_K;
}

} // namespace

extern "C" uint32_t gs_kmeans_padded_width(uint32_t w) { return kmeans_padded_width(w); }

extern "C" uint32_t gs_kmeans_default_slices(uint32_t n, uint32_t w, uint32_t k) {
    if (!kmeans_shape_ok(n, w, k)) return 0;
    // 1024 workgroups (four per CU) keep the chip busy; below that the centroids are cut, into slices of 64 rows at least
    const uint32_t blocks = gs_div_up(n, (uint64_t)GS_BLOCK * kmeans_points_per_lane(kmeans_padded_width(w)));
    if (blocks >= 1024u) return 1;
    const uint32_t want = gs_div_up(1024u, blocks), most = gs_div_up(k, 64u);
    return want < most ? want : most;
}

extern "C" int32_t gs_kmeans_assign(uint32_t n, uint32_t w, uint32_t k, const int32_t *q, const int32_t *cent, uint32_t k_slices,
                                    uint64_t *keys, int32_t *labels, uint32_t *n_changed, gs_stream_t stream) {
    GS_CHECK_ARG(kmeans_shape_ok(n, w, k), "need 1 <= n < 2^31, 1 <= w <= 64 and 1 <= k <= 2^20");
    GS_CHECK_ARG(q && cent && labels && n_changed, "null pointer");
    GS_CHECK_ARG(k_slices >= 1 && k_slices <= k && k_slices <= 65535u, "need 1 <= k_slices <= min(k, 65535)");
    GS_CHECK_ARG(k_slices == 1 || keys, "k_slices > 1 needs the key buffer");
    GS_CHECK_ARG((uintptr_t)cent % 16u == 0, "cent must be 16-byte aligned (its rows are read four words at a time)");
    const hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(n_changed, 0, sizeof(uint32_t), s) != hipSuccess ||
        (k_slices > 1 && hipMemsetAsync(keys, 0xFF, (size_t)n * sizeof(uint64_t), s) != hipSuccess)) {
        gs_set_error("%s: hipMemsetAsync failed", __func__);
        return 2;
    }
    const uint32_t *uq = (const uint32_t *)q, *uc = (const uint32_t *)cent;
    unsigned long long *ukeys = (unsigned long long *)keys;
    switch (kmeans_padded_width(w)) {
    case 4: kmeans_launch_assign<4>(n, w, k, k_slices, uq, uc, ukeys, labels, n_changed, s); break;
    case 8: kmeans_launch_assign<8>(n, w, k, k_slices, uq, uc, ukeys, labels, n_changed, s); break;
    case 16: kmeans_launch_assign<16>(n, w, k, k_slices, uq, uc, ukeys, labels, n_changed, s); break;
    case 32: kmeans_launch_assign<32>(n, w, k, k_slices, uq, uc, ukeys, labels, n_changed, s); break;
    case 48: kmeans_launch_assign<48>(n, w, k, k_slices, uq, uc, ukeys, labels, n_changed, s); break;
    default: kmeans_launch_assign<64>(n, w, k, k_slices, uq, uc, ukeys, labels, n_changed, s); break;
    }
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_kmeans_update(uint32_t n, uint32_t w, uint32_t k, const int32_t *q, const int32_t *labels, uint64_t *sums,
                                    uint32_t *counts, int32_t *cent, gs_stream_t stream) {
    GS_CHECK_ARG(kmeans_shape_ok(n, w, k), "need 1 <= n < 2^31, 1 <= w <= 64 and 1 <= k <= 2^20");
    GS_CHECK_ARG(q && labels && sums && counts && cent, "null pointer");
    const hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, (size_t)k * w * sizeof(uint64_t), s) != hipSuccess ||
        hipMemsetAsync(counts, 0, (size_t)k * sizeof(uint32_t), s) != hipSuccess) {
        gs_set_error("%s: hipMemsetAsync failed", __func__);
        return 2;
    }
    const uint64_t elements = (uint64_t)n * w; // < 2^37: at most 2^29 workgroups
    hipLaunchKernelGGL(kmeans_accumulate_kernel, dim3(gs_div_up(elements, GS_BLOCK)), dim3(GS_BLOCK), 0, s, n, w, k, (const uint32_t *)q, labels,
                       (unsigned long long *)sums, counts);
    hipLaunchKernelGGL(kmeans_finalise_kernel, dim3(gs_div_up((uint64_t)k * w, GS_BLOCK)), dim3(GS_BLOCK), 0, s, w, kmeans_padded_width(w), k,
                       (const unsigned long long *)sums, (const uint32_t *)counts, (uint32_t *)cent);
    GS_CHECK_LAUNCH();
    return 0;
}
