// knn.hip -- exact k nearest neighbours of 3-D float32 points over a uniform grid (gfx950).
//
// The reference's trainers size their initial splats from `knn(points, 4)` (examples/utils.py:142-146: a copy to the host,
// sklearn's NearestNeighbors on one core, a copy back).  Here the algorithm is the library's own, defined by the numpy code
// gscodec_studio_amd/knn_reference.py: a grid over the 1 % .. 99 % box of the points with clamped (infinite) border cells,
// and per query a search over rings of cells that stops once the K-th distance is certified by the faces of the searched
// block.  The result is exact: the K nearest by (float32 d^2, index).  No atomics: bit-identical from run to run.
//
//   gs_knn_cells         cell id of every point, (double(p) - lo) / h in float64 like the definition: the sort keys
//   gs_knn_finish_grid   after the radix sort of (id, index): the cell-sorted float4 copy (xyz, index bits in w) and
//                        cell_starts (one lane per cell, a binary search over the sorted ids)
//   gs_knn_search        one lane per query, queries in cell-sorted order: the lanes of a wave walk the same rows of cells, so
//                        their loads of cell_starts and of the points coalesce or broadcast.  The K best live in registers
//                        (K padded to 4 / 8 / 16, an unrolled compare-and-shift insertion, no runtime-indexed array); rows
//                        are written at the query's original index; optionally the trainers' log scale in the epilogue.
#include "gs_common.h"

namespace {

constexpr uint32_t KNN_MAX_K = 16;
constexpr uint32_t KNN_MAX_R = 1024;
constexpr uint32_t KNN_NO_INDEX = 0x7FFFFFFFu;

struct KnnGrid {
    double lo[3], h;
    int32_t R[3];
};

// step 3 of the definition; IEEE subtract and divide in float64: the ids equal numpy's
GS_DEV int32_t knn_cell_coord(float p, double lo, double h, int32_t R) {
    const double v = floor(((double)p - lo) / h);
    return v < 0.0 ? 0 : (v > (double)(R - 1) ? R - 1 : (int32_t)v);
}

__global__ void __launch_bounds__(GS_BLOCK) knn_cells_kernel(uint32_t n, const float *__restrict__ xyz, KnnGrid g,
                                                             int64_t *__restrict__ cell_ids, int32_t *__restrict__ ids) {
    const uint32_t i = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t cx = knn_cell_coord(xyz[3ull * i], g.lo[0], g.h, g.R[0]);
    const int32_t cy = knn_cell_coord(xyz[3ull * i + 1], g.lo[1], g.h, g.R[1]);
    const int32_t cz = knn_cell_coord(xyz[3ull * i + 2], g.lo[2], g.h, g.R[2]);
    cell_ids[i] = (int64_t)((cz * g.R[1] + cy) * g.R[0] + cx); // < 2^30 cells
    ids[i] = (int32_t)i;
}

__global__ void __launch_bounds__(GS_BLOCK) knn_gather_kernel(uint32_t n, const float *__restrict__ xyz, const int32_t *__restrict__ order,
                                                              float4 *__restrict__ sorted) {
    const uint32_t p = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint32_t i = (uint32_t)order[p];
    if (i >= n) return; // (an order that is no permutation reads nothing out of bounds)
    sorted[p] = make_float4(xyz[3ull * i], xyz[3ull * i + 1], xyz[3ull * i + 2], __uint_as_float(i));
}

// cell_starts[c] = the number of sorted ids below c, for c in [0, ncells]
__global__ void __launch_bounds__(GS_BLOCK) knn_cell_starts_kernel(uint32_t n, uint32_t ncells, const int64_t *__restrict__ sorted_ids,
                                                                   int32_t *__restrict__ cell_starts) {
    const uint32_t c = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (c > ncells) return;
    uint32_t a = 0, b = n; // the answer is in [a, b]
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2u;
        if (sorted_ids[mid] < (int64_t)c) a = mid + 1u; else b = mid;
    }
    cell_starts[c] = (int32_t)a;
}

// (d2, i) < (bd, bi): indices are distinct, so this is a strict total order; the empty slots (inf, KNN_NO_INDEX) come last
GS_DEV bool knn_before(float d2, uint32_t i, float bd, uint32_t bi) { return d2 < bd || (d2 == bd && i < bi); }

template <uint32_t KP>
GS_DEV void knn_insert(float (&bd)[KP], uint32_t (&bi)[KP], float d2, uint32_t i) {
#pragma unroll
    for (uint32_t j = KP - 1u; j > 0u; --j) { // slot j takes its left neighbour, the candidate, or stays
        const bool left = knn_before(d2, i, bd[j - 1u], bi[j - 1u]);
        const bool here = knn_before(d2, i, bd[j], bi[j]);
        bd[j] = left ? bd[j - 1u] : (here ? d2 : bd[j]);
        bi[j] = left ? bi[j - 1u] : (here ? i : bi[j]);
    }
    const bool first = knn_before(d2, i, bd[0], bi[0]);
    bd[0] = first ? d2 : bd[0];
    bi[0] = first ? i : bi[0];
}

template <uint32_t KP>
__global__ void __launch_bounds__(GS_BLOCK) knn_search_kernel(uint32_t n, uint32_t m, uint32_t K, const float4 *__restrict__ pts,
                                                              const int32_t *__restrict__ cell_starts, const float4 *__restrict__ queries,
                                                              KnnGrid g, float *__restrict__ dist, int64_t *__restrict__ idx,
                                                              float *__restrict__ log_scales, float init_scale) {
    const uint32_t t = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (t >= m) return;
    const float4 q = queries[t];
    const uint32_t row = __float_as_uint(q.w);
    if (row >= m) return; // (a query list that carries no row index writes nothing)
    const int32_t Rx = g.R[0], Ry = g.R[1], Rz = g.R[2];
    const int32_t cx = knn_cell_coord(q.x, g.lo[0], g.h, Rx), cy = knn_cell_coord(q.y, g.lo[1], g.h, Ry),
                  cz = knn_cell_coord(q.z, g.lo[2], g.h, Rz);
    // the absolute slack of the face distances (step 4): 2^-40 of the coordinates that enter them
    const double slack_x = 0x1p-40 * (fabs((double)q.x) + (fabs(g.lo[0]) + Rx * g.h));
    const double slack_y = 0x1p-40 * (fabs((double)q.y) + (fabs(g.lo[1]) + Ry * g.h));
    const double slack_z = 0x1p-40 * (fabs((double)q.z) + (fabs(g.lo[2]) + Rz * g.h));
    float bd[KP];
    uint32_t bi[KP];
#pragma unroll
    for (uint32_t j = 0; j < KP; ++j) {
        bd[j] = __builtin_inff();
        bi[j] = KNN_NO_INDEX;
    }
    for (int32_t r = 0;; ++r) {
        for (int32_t dz = -r; dz <= r; ++dz) {
            const int32_t z = cz + dz;
            if (z < 0 || z >= Rz) continue;
            for (int32_t dy = -r; dy <= r; ++dy) {
                const int32_t y = cy + dy;
                if (y < 0 || y >= Ry) continue;
                const int32_t base = (z * Ry + y) * Rx;
                const bool shell = dz == -r || dz == r || dy == -r || dy == r; // the whole x-row is at distance r
                // a row of the shell is one run of sorted positions; inside, the two cells at x = cx -+ r are a run each
                for (int32_t side = 0; side < (shell ? 1 : 2); ++side) {
                    int32_t x0, x1;
                    if (shell) {
                        x0 = max(cx - r, 0);
                        x1 = min(cx + r, Rx - 1);
                    } else {
                        x0 = x1 = side ? cx + r : cx - r;
                        if (x0 < 0 || x0 >= Rx) continue;
                    }
                    const int32_t p1 = cell_starts[base + x1 + 1];
                    for (int32_t p = cell_starts[base + x0]; p < p1; ++p) {
                        GS_FP_STRICT
                        const float4 c = pts[p];
                        const float dx = q.x - c.x, dy_ = q.y - c.y, dz_ = q.z - c.z;
                        const float d2 = (dx * dx + dy_ * dy_) + dz_ * dz_;
                        const uint32_t i = __float_as_uint(c.w);
                        if (knn_before(d2, i, bd[KP - 1u], bi[KP - 1u])) knn_insert<KP>(bd, bi, d2, i);
                    }
                }
            }
        }
        // the least distance to a face of the block [c - r, c + r] that is no grid border
        double b = __builtin_inf();
        if (cx - r > 0) b = fmin(b, (double)q.x - (g.lo[0] + (cx - r) * g.h) - slack_x);
        if (cx + r + 1 < Rx) b = fmin(b, (g.lo[0] + (cx + r + 1) * g.h) - (double)q.x - slack_x);
        if (cy - r > 0) b = fmin(b, (double)q.y - (g.lo[1] + (cy - r) * g.h) - slack_y);
        if (cy + r + 1 < Ry) b = fmin(b, (g.lo[1] + (cy + r + 1) * g.h) - (double)q.y - slack_y);
        if (cz - r > 0) b = fmin(b, (double)q.z - (g.lo[2] + (cz - r) * g.h) - slack_z);
        if (cz + r + 1 < Rz) b = fmin(b, (g.lo[2] + (cz + r + 1) * g.h) - (double)q.z - slack_z);
        if (b == __builtin_inf()) break; // the block is the grid: r < KNN_MAX_R ends the loop
        float kth = bd[0];
#pragma unroll
        for (uint32_t j = 1; j < KP; ++j) kth = j == K - 1u ? bd[j] : kth;
        b = fmax(b, 0.0);
        if ((double)kth < b * b * (1.0 - 0x1p-20)) break; // strictly: nothing outside the block ties with the K-th
    }
    if (dist) {
#pragma unroll
        for (uint32_t j = 0; j < KP; ++j)
            if (j < K) {
                dist[(uint64_t)row * K + j] = sqrtf(bd[j]);
                idx[(uint64_t)row * K + j] = (int64_t)bi[j];
            }
    }
    if (log_scales) { // log(sqrt(mean of d^2 over the K - 1 neighbours) * init_scale): the sum and what follows in float64
        double s = 0.0;
#pragma unroll
        for (uint32_t j = 1; j < KP; ++j) s += j < K ? (double)bd[j] : 0.0;
        const float v = (float)log(sqrt(s / (double)(K - 1u)) * (double)init_scale);
        log_scales[3ull * row] = v;
        log_scales[3ull * row + 1] = v;
        log_scales[3ull * row + 2] = v;
    }
}

bool knn_grid_ok(const double *box, uint32_t rx, uint32_t ry, uint32_t rz) {
    return box && box[3] > 0.0 && rx >= 1 && rx <= KNN_MAX_R && ry >= 1 && ry <= KNN_MAX_R && rz >= 1 && rz <= KNN_MAX_R;
}

KnnGrid knn_grid(const double *box, uint32_t rx, uint32_t ry, uint32_t rz) { // box: host memory, copied into the kernel arguments
    KnnGrid g;
    g.lo[0] = box[0], g.lo[1] = box[1], g.lo[2] = box[2], g.h = box[3];
    g.R[0] = (int32_t)rx, g.R[1] = (int32_t)ry, g.R[2] = (int32_t)rz;
    return g;
}

} // namespace

extern "C" int32_t gs_knn_cells(uint32_t n, const float *xyz, const double *box, uint32_t rx, uint32_t ry, uint32_t rz, int64_t *cell_ids,
                                int32_t *ids, gs_stream_t stream) {
    GS_CHECK_ARG(n >= 1 && n < (1u << 31), "need 1 <= n < 2^31");
    GS_CHECK_ARG(knn_grid_ok(box, rx, ry, rz), "need the box, h > 0 and 1 <= R <= 1024 per axis");
    GS_CHECK_ARG(xyz && cell_ids && ids, "null pointer");
    hipLaunchKernelGGL(knn_cells_kernel, dim3(gs_div_up(n, GS_BLOCK)), dim3(GS_BLOCK), 0, (hipStream_t)stream, n, xyz,
                       knn_grid(box, rx, ry, rz), cell_ids, ids);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_knn_finish_grid(uint32_t n, uint32_t ncells, const float *xyz, const int64_t *sorted_ids, const int32_t *order,
                                      float *sorted_xyzi, int32_t *cell_starts, gs_stream_t stream) {
    GS_CHECK_ARG(n >= 1 && n < (1u << 31), "need 1 <= n < 2^31");
    GS_CHECK_ARG(ncells <= (1u << 30), "at most 2^30 cells");
    GS_CHECK_ARG(xyz && order && sorted_xyzi, "null pointer");
    GS_CHECK_ARG((uintptr_t)sorted_xyzi % 16u == 0, "sorted_xyzi must be 16-byte aligned");
    GS_CHECK_ARG(ncells == 0 || (sorted_ids && cell_starts), "cell_starts needs the sorted ids");
    hipLaunchKernelGGL(knn_gather_kernel, dim3(gs_div_up(n, GS_BLOCK)), dim3(GS_BLOCK), 0, (hipStream_t)stream, n, xyz, order,
                       (float4 *)sorted_xyzi);
    if (ncells)
        hipLaunchKernelGGL(knn_cell_starts_kernel, dim3(gs_div_up((uint64_t)ncells + 1u, GS_BLOCK)), dim3(GS_BLOCK), 0, (hipStream_t)stream, n,
                           ncells, sorted_ids, cell_starts);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_knn_search(uint32_t n, uint32_t m, uint32_t K, const float *sorted_xyzi, const int32_t *cell_starts,
                                 const float *queries_xyzi, const double *box, uint32_t rx, uint32_t ry, uint32_t rz, float *dist,
                                 int64_t *idx, float *log_scales, float init_scale, gs_stream_t stream) {
    GS_CHECK_ARG(n >= 1 && n < (1u << 31) && m >= 1 && m < (1u << 31), "need 1 <= n, m < 2^31");
    GS_CHECK_ARG(K >= 1 && K <= KNN_MAX_K && K <= n, "need 1 <= K <= min(16, n)");
    GS_CHECK_ARG(knn_grid_ok(box, rx, ry, rz), "need the box, h > 0 and 1 <= R <= 1024 per axis");
    GS_CHECK_ARG(sorted_xyzi && cell_starts && queries_xyzi, "null pointer");
    GS_CHECK_ARG((uintptr_t)sorted_xyzi % 16u == 0 && (uintptr_t)queries_xyzi % 16u == 0, "the point arrays must be 16-byte aligned");
    GS_CHECK_ARG((dist == nullptr) == (idx == nullptr) && (dist || log_scales), "dist and idx go together; nothing to write");
    GS_CHECK_ARG(!log_scales || K >= 2, "log_scales is a mean over K - 1 neighbours: K >= 2");
    const KnnGrid g = knn_grid(box, rx, ry, rz);
    const dim3 grid(gs_div_up(m, GS_BLOCK)), block(GS_BLOCK);
    const float4 *p = (const float4 *)sorted_xyzi, *q = (const float4 *)queries_xyzi;
    const hipStream_t s = (hipStream_t)stream;
    switch (K <= 4 ? 4 : (K <= 8 ? 8 : 16)) { // the register array the K best live in
    case 4: hipLaunchKernelGGL(knn_search_kernel<4>, grid, block, 0, s, n, m, K, p, cell_starts, q, g, dist, idx, log_scales, init_scale); break;
    case 8: hipLaunchKernelGGL(knn_search_kernel<8>, grid, block, 0, s, n, m, K, p, cell_starts, q, g, dist, idx, log_scales, init_scale); break;
    default: hipLaunchKernelGGL(knn_search_kernel<16>, grid, block, 0, s, n, m, K, p, cell_starts, q, g, dist, idx, log_scales, init_scale); break;
    }
    GS_CHECK_LAUNCH();
    return 0;
}
