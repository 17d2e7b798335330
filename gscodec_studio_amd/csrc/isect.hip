// isect.hip -- R3/R4: gaussian/tile intersection, prefix sums, offset encode (gfx950).
//
// Replaces gsplat/cuda/csrc/isect_tiles.cu:16-104 (count + emit passes), the
// torch::cumsum between them (isect_tiles.cu:199) and isect_offset_encode
// (isect_tiles.cu:308-354).  The 64-bit radix sort lives in radix_sort.hip.
//
// All outputs of this file are integers derived from fp32 inputs with IEEE
// (correctly rounded) division / floor / ceil, so they are bit-exact against the
// oracle.  The file is compiled with -ffp-contract=off.
#include "gs_common.h"
#include "scan_dev.h"

#include <atomic>

namespace {

__global__ void __launch_bounds__(GS_BLOCK) isect_count_kernel(
    uint32_t n_elems, const float *__restrict__ means2d, uint32_t s_m2, const int32_t *__restrict__ radii,
    float tile_size, int32_t tw, int32_t th, int32_t *__restrict__ tiles_per_gauss) {
    uint32_t i = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (i >= n_elems) return;
    int32_t r = radii[i];
    int32_t cnt = 0;
    if (r > 0) {
        float2 m = *reinterpret_cast<const float2 *>(means2d + (size_t)i * s_m2);
        TileBox b = tile_box(m.x, m.y, r, tile_size, tw, th);
        cnt = (b.y1 - b.y0) * (b.x1 - b.x0);
    }
    tiles_per_gauss[i] = cnt;
}

// Depth keys for the splat-level pre-sort: (float_bits(depth) << 32) | element for visible
// elements, a maximal positive key for culled ones (they sort last and emit nothing).
__global__ void __launch_bounds__(GS_BLOCK) isect_depth_keys_kernel(
    uint32_t n_elems, const int32_t *__restrict__ radii, const float *__restrict__ depths,
    int64_t *__restrict__ keys, int32_t *__restrict__ vals) {
    uint32_t i = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (i >= n_elems) return;
    uint32_t d = radii[i] > 0 ? (uint32_t)__float_as_int(depths[i]) & 0x7fffffffu : 0x7fffffffu;
    keys[i] = (int64_t)(((uint64_t)d << 32) | (uint64_t)i);
    vals[i] = (int32_t)i;
}

// isect_count_kernel + isect_depth_keys_kernel in one launch (the sorted path needs both)
// block_sums (optional): the block's number of intersections.  Their sum is n_isects -- available right after THIS kernel,
// ~100 us of GPU work (depth pre-sort, prefix sum, SH colours) before the pipeline needs it on the host: the caller copies
// the partial sums to pinned memory here and adds them up on the host, so the one host read-back of the pipeline
// (isect_tiles.cu:200 in the reference) no longer leaves the GPU idle while the host wakes up and queues the rest.
// hist (optional): the digit histogram of the depth pre-sort's FIRST pass for this block's 1024 keys (digit = low 8 bits of
// the depth bits, culled keys not counted), in the sort's own [256][n_blocks] layout -- the sort then skips that launch.
constexpr int COUNT_ITEMS = 4; // elements per thread: a block covers the 1024 keys of one sort block
__global__ void __launch_bounds__(GS_BLOCK) isect_count_keys_kernel(
    uint32_t n_elems, const float *__restrict__ means2d, uint32_t s_m2, const int32_t *__restrict__ radii,
    const float *__restrict__ depths, float tile_size, int32_t tw, int32_t th,
    int32_t *__restrict__ tiles_per_gauss, int64_t *__restrict__ keys, int32_t *__restrict__ vals, int32_t *__restrict__ block_sums,
    uint32_t *__restrict__ hist, uint32_t n_blocks, const uint64_t *__restrict__ split) {
    __shared__ int32_t s_sum[GS_BLOCK / GS_WAVE], s_vis[GS_BLOCK / GS_WAVE];
    __shared__ uint32_t s_hist[256];
    __shared__ uint64_t s_split[GS_PRESORT_BUCKETS];
    if (hist != nullptr) s_hist[threadIdx.x] = 0u;
    if (split != nullptr) s_split[threadIdx.x] = split[threadIdx.x]; // bucketed pre-sort: digit = bucket of the whole key
    __syncthreads();
    int32_t cnt_sum = 0, vis_sum = 0;
#pragma unroll
    for (int k = 0; k < COUNT_ITEMS; ++k) {
        const uint32_t i = (blockIdx.x * COUNT_ITEMS + k) * GS_BLOCK + threadIdx.x;
        if (i >= n_elems) continue;
        const int32_t r = radii[i];
        uint32_t d = 0x7fffffffu;
        int32_t cnt = 0;
        if (r > 0) {
            if (means2d != nullptr) { // (uniform; NULL: tiles_per_gauss holds the counts already -- gs_projection_rows_fwd made them)
                float2 m = *reinterpret_cast<const float2 *>(means2d + (size_t)i * s_m2);
                TileBox b = tile_box(m.x, m.y, r, tile_size, tw, th);
                cnt = (b.y1 - b.y0) * (b.x1 - b.x0);
            }
            d = (uint32_t)__float_as_int(depths[i]) & 0x7fffffffu;
        }
        if (means2d != nullptr) tiles_per_gauss[i] = cnt;
        const uint64_t key = ((uint64_t)d << 32) | (uint64_t)i;
        keys[i] = (int64_t)key;
        if (vals != nullptr) vals[i] = (int32_t)i; // (NULL: the bucketed pre-sort reads the element off the key's low half)
        cnt_sum += cnt;
        vis_sum += r > 0 ? 1 : 0;
        if (hist != nullptr && d != 0x7fffffffu) atomicAdd(&s_hist[split != nullptr ? gs_bucket_of(s_split, key) : (d & 0xffu)], 1u);
    }
    if (block_sums != nullptr) { // (block-uniform)
        int32_t v = cnt_sum, u = vis_sum;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            v += __shfl_xor(v, off, 64);
            u += __shfl_xor(u, off, 64);
        }
        if ((threadIdx.x & 63u) == 0u) {
            s_sum[threadIdx.x >> 6] = v;
            s_vis[threadIdx.x >> 6] = u;
        }
        __syncthreads();
        if (threadIdx.x == 0) // (intersections, visible elements) as ONE 8-byte store: they reach the host together
            reinterpret_cast<int2 *>(block_sums)[blockIdx.x] = make_int2(s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3], s_vis[0] + s_vis[1] + s_vis[2] + s_vis[3]);
    }
    if (hist != nullptr) {
        __syncthreads();
        hist[(size_t)threadIdx.x * n_blocks + blockIdx.x] = s_hist[threadIdx.x];
    }
}

__global__ void __launch_bounds__(GS_BLOCK) gather_i32_kernel(
    uint32_t n, const int32_t *__restrict__ src, const int32_t *__restrict__ idx, int32_t *__restrict__ out) {
    uint32_t i = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (i < n) out[i] = src[idx[i]];
}

// Wave-cooperative emission.  A wave owns a few consecutive positions of the emission order, whose pairs
// form ONE contiguous output range [cum[first-1], cum[last]).  The lanes first park their splat's
// record (output start, tile box, key base, id) in LDS, then walk the output range 64 slots at a time:
// slot o finds its owner by a binary search over the starts and derives its tile from its
// offset inside the owner's box.  Stores are fully coalesced (the one-thread-per-splat loop wrote 12 B
// at ~160 B strides: 51 us for 4 M pairs at config 2, 2.7x the compulsory traffic).
struct EmitRec {
    int64_t key_base; // camera bits | depth bits
    int32_t id;       // flatten id
    int32_t x0, y0, w;
};

// A wave owns EMIT_SPW consecutive positions of the emission order (16, not 64: the emission order is the depth order, so the big near splats
// sit next to each other and a 64-splat wave could own thousands of pairs while most own a few hundred -- the kernel
// lasted as long as that wave: 37 us at config 2 against 24 us with 16).
#ifndef GS_EMIT_SPW
#define GS_EMIT_SPW 16
#endif
constexpr uint32_t EMIT_SPW = GS_EMIT_SPW;
constexpr uint32_t EMIT_WAVES = GS_BLOCK / GS_WAVE;

// MODE 0: 64-bit ids + flatten ids; 1 (compact): 32-bit (camera, tile) key + flatten id for the 32-bit pair sort
// (gs_sort_isect_pairs rebuilds the 64-bit id with the depth bits in its last pass); 2 (packed): ONE 32-bit word per pair,
// key << pos_bits | emission position -- the position is the splat's depth rank, nothing else has to ride through the sort.

// The emission record of element `e` at position `pos` of the emission order (has == false: the position holds no element).
// Radius and mean go out together; a culled element leaves a record that owns no pair.
template <int MODE>
GS_DEV EmitRec emit_rec_of(bool has, uint32_t e, uint32_t pos, uint32_t N, const int64_t *__restrict__ camera_ids,
                           const float *__restrict__ means2d, uint32_t s_m2, const int32_t *__restrict__ radii,
                           const float *__restrict__ depths, float tile_size, int32_t tw, int32_t th, uint32_t tile_n_bits) {
    EmitRec rec = {0, 0, 0, 0, 1};
    int32_t r = 0;
    float2 m = make_float2(0.f, 0.f);
    if (has) {
        r = radii[e];
        m = *reinterpret_cast<const float2 *>(means2d + (size_t)e * s_m2);
    }
    if (r > 0) {
        const TileBox b = tile_box(m.x, m.y, r, tile_size, tw, th);
        const int64_t cid = camera_ids != nullptr ? camera_ids[e] : (int64_t)(e / N);
        // raw IEEE bits of the (positive) depth, sign-extended like the reference's
        // (int64_t)*(int32_t*)&depth  (isect_tiles.cu:91)
        rec.key_base = MODE != 0 ? (cid << tile_n_bits) : ((cid << (32 + tile_n_bits)) | (int64_t)__float_as_int(depths[e]));
        rec.id = MODE == 2 ? (int32_t)pos : (int32_t)e; // (packed: the emission position)
        rec.x0 = b.x0;
        rec.y0 = b.y0;
        rec.w = max(b.x1 - b.x0, 1);
    }
    return rec;
}

// A wave writes the `total` pairs of its EMIT_SPW records to the output range that begins at out0, 64 slots at a time.
// wstart: EMIT_SPW + 1 starts (last = total), published to the wave before the call.
template <int MODE>
GS_DEV void expand_pairs(const EmitRec *wrec, const int32_t *wstart, int32_t total, int64_t out0, int32_t tw,
                         int64_t *__restrict__ isect_ids, uint32_t *__restrict__ keys32, int32_t *__restrict__ flatten_ids,
                         uint32_t pos_bits) {
    for (int32_t t = (int32_t)(threadIdx.x % GS_WAVE); t < total; t += GS_WAVE) {
        // largest s with start[s] <= t (zero-count lanes share their successor's start and are skipped)
        int32_t sidx = 0;
#pragma unroll
        for (int step = EMIT_SPW / 2; step > 0; step >>= 1)
            if (wstart[sidx + step] <= t) sidx += step;
        const EmitRec o = wrec[sidx];
        const int32_t k = t - wstart[sidx];
        // k / w without the ~30-instruction integer division: float quotient, then one exact correction step (the float
        // result is off by at most one for any k < 2^24; k < tiles of the grid, which emit_check_args bounds)
        int32_t dy = (int32_t)(((float)k + 0.5f) * __builtin_amdgcn_rcpf((float)o.w));
        int32_t dx = k - dy * o.w;
        if (dx < 0) { dy -= 1; dx += o.w; }
        else if (dx >= o.w) { dy += 1; dx -= o.w; }
        const int64_t tile_id = (int64_t)(o.y0 + dy) * tw + (o.x0 + dx);
        if (MODE == 2) keys32[out0 + t] = ((uint32_t)(o.key_base | tile_id) << pos_bits) | (uint32_t)o.id;
        else if (MODE == 1) keys32[out0 + t] = (uint32_t)(o.key_base | tile_id);
        else isect_ids[out0 + t] = o.key_base | (tile_id << 32);
        if (MODE != 2) flatten_ids[out0 + t] = o.id;
    }
}

template <bool COMPACT>
__global__ void __launch_bounds__(GS_BLOCK) isect_emit_kernel(
    uint32_t n_elems, uint32_t N, const int32_t *__restrict__ perm, const uint32_t *__restrict__ n_valid,
    const int64_t *__restrict__ camera_ids,
    const float *__restrict__ means2d, uint32_t s_m2, const int32_t *__restrict__ radii,
    const float *__restrict__ depths, const int64_t *__restrict__ cum_tiles,
    float tile_size, int32_t tw, int32_t th, uint32_t tile_n_bits,
    int64_t *__restrict__ isect_ids, uint32_t *__restrict__ keys32, int32_t *__restrict__ flatten_ids) {
    // `pos` = position in the emission order (identity, or depth-sorted when perm is given);
    // `i` = the element it refers to.  cum_tiles is indexed by position.
    __shared__ EmitRec s_rec[EMIT_WAVES * EMIT_SPW];
    __shared__ int32_t s_start[EMIT_WAVES * (EMIT_SPW + 1)]; // SPW + 1 starts per wave (last = total)
    const uint32_t lane = threadIdx.x % GS_WAVE, wave = threadIdx.x / GS_WAVE;
    const uint32_t wave_first = (blockIdx.x * EMIT_WAVES + wave) * EMIT_SPW;
    if (wave_first >= n_elems) return; // wave-uniform
    if (n_valid != nullptr && wave_first >= *n_valid) return; // behind the valid prefix (cum_tiles is not defined there)
    const uint32_t pos = wave_first + lane; // lanes >= EMIT_SPW carry no splat
    const uint32_t wave_last = min(wave_first + EMIT_SPW, n_elems) - 1;
    const int64_t out0 = (wave_first == 0) ? 0 : cum_tiles[wave_first - 1];
    const int64_t out1 = cum_tiles[wave_last];
    if (out1 == out0) return; // nothing visible in this wave (wave-uniform)
    EmitRec *wrec = s_rec + wave * EMIT_SPW;
    int32_t *wstart = s_start + wave * (EMIT_SPW + 1);
    const int32_t total = (int32_t)(out1 - out0);
    if (lane < EMIT_SPW) {
        // positions behind *n_valid hold no element (perm is only defined for the kept ones)
        const bool has = pos < n_elems && (n_valid == nullptr || pos < *n_valid);
        const uint32_t i = has ? (perm != nullptr ? (uint32_t)perm[pos] : pos) : 0u;
        wrec[lane] = emit_rec_of<COMPACT ? 1 : 0>(has, i, pos, N, camera_ids, means2d, s_m2, radii, depths, tile_size, tw, th, tile_n_bits);
        wstart[lane] = pos < n_elems ? (int32_t)(((pos == 0) ? 0 : cum_tiles[pos - 1]) - out0) : total;
    }
    if (lane == 0) wstart[EMIT_SPW] = total;
    __builtin_amdgcn_wave_barrier();
    expand_pairs<COMPACT ? 1 : 0>(wrec, wstart, total, out0, tw, isect_ids, keys32, flatten_ids, 0u);
}

// Emission for the PRE-SORTED path with the prefix scan folded in (round 3: the two launches of gs_cumsum_gather_i32 and the
// cum_tiles array are gone).  A workgroup owns EMIT_SCAN_TILE (= 128) consecutive positions of the emission order:
//   * its output offset = the sum of its predecessors' group sums (group_sums[g] = tiles of positions [128 g, 128 (g+1)),
//     left behind by the LAST pass of the depth pre-sort -- gs_presort_buckets / gs_sort_pairs_u64_i32_drop: side_sums);
//   * tile count, radius and mean of its positions are gathered through perm in ONE phase; the inclusive scan of the
//     counts and the emission records of all 128 positions live in LDS;
//   * its four waves then emit groups of EMIT_SPW positions exactly like isect_emit_kernel.
constexpr uint32_t EMIT_SCAN_SHIFT = 7; // 128 positions per workgroup: two groups of EMIT_SPW per wave (512: 58 us for 572
                                        // workgroups of eight sequential groups per wave -- too few waves in flight; the
                                        // one-group-per-wave kernel above needed 19 us + 15 us of prefix-sum launches)
constexpr uint32_t EMIT_SCAN_TILE = 1u << EMIT_SCAN_SHIFT;
static_assert(EMIT_SCAN_TILE <= GS_BLOCK && EMIT_SCAN_TILE % EMIT_SPW == 0, "one position per thread");

// MODE: see emit_rec_of
template <int MODE>
__global__ void __launch_bounds__(GS_BLOCK) isect_emit_scan_kernel(
    uint32_t n_elems, uint32_t N, const int32_t *__restrict__ perm, const uint32_t *__restrict__ n_valid,
    const int64_t *__restrict__ camera_ids, const float *__restrict__ means2d, uint32_t s_m2, const int32_t *__restrict__ radii,
    const float *__restrict__ depths, const int32_t *__restrict__ tiles_per_gauss, const uint32_t *__restrict__ group_sums,
    const int64_t *__restrict__ group_prefix, float tile_size, int32_t tw, int32_t th, uint32_t tile_n_bits,
    int64_t *__restrict__ isect_ids, uint32_t *__restrict__ keys32, int32_t *__restrict__ flatten_ids, uint32_t pos_bits) {
    __shared__ int32_t s_cum[EMIT_SCAN_TILE + 1]; // s_cum[j] = tiles of the block's positions [0, j)
    __shared__ int64_t s_red[GS_BLOCK / GS_WAVE];
    __shared__ int32_t s_wsum[GS_BLOCK / GS_WAVE];
    __shared__ EmitRec s_rec[EMIT_SCAN_TILE]; // the record of EVERY position of the block, gathered in one phase
    __shared__ int32_t s_start[EMIT_WAVES * (EMIT_SPW + 1)];
    const uint32_t tid = threadIdx.x, lane = tid % GS_WAVE, wave = tid / GS_WAVE;
    const uint32_t nv = n_valid != nullptr ? min(n_elems, *n_valid) : n_elems;
    const uint32_t block_first = blockIdx.x * EMIT_SCAN_TILE;
    if (block_first >= nv) return; // (block-uniform) nothing to emit here or behind
    // ---- offset of this block in the output: its predecessors' group sums
    // (every block adds up its predecessors itself -- quadratic, fine for the few thousand groups of a million splats; the
    // caller hands over the inclusive prefix instead when there are more)
    int64_t pre = 0;
    if (group_prefix != nullptr) pre = (tid == 0 && blockIdx.x > 0) ? group_prefix[blockIdx.x - 1] : 0;
    else
        for (uint32_t g = tid; g < blockIdx.x; g += GS_BLOCK) pre += (int64_t)group_sums[g];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) pre += __shfl_xor(pre, off, 64);
    if (lane == 0) s_red[wave] = pre;
    // ---- my position (threads beyond the tile only help with the offset above)
    int32_t c = 0, e = -1;
    if (tid < EMIT_SCAN_TILE) {
        const uint32_t pos = block_first + tid;
        e = pos < nv ? (perm != nullptr ? perm[pos] : (int32_t)pos) : -1;
        // the three gathers that hang off the element index go out together (they used to be two dependent phases: the tile
        // count here, radius and mean inside the per-group loop below -- once per group and wave)
        if (e >= 0) c = tiles_per_gauss[e];
        s_rec[tid] = emit_rec_of<MODE>(e >= 0, (uint32_t)e, pos, N, camera_ids, means2d, s_m2, radii, depths, tile_size, tw, th, tile_n_bits);
    }
    // (the cross-wave part of the scan stays here: its two barriers also publish s_red and s_rec)
    const int32_t inc = wave_inclusive_scan(c);
    if (lane == GS_WAVE - 1) s_wsum[wave] = inc;
    __syncthreads();
    int32_t wbase = 0;
#pragma unroll
    for (int w = 0; w < GS_BLOCK / GS_WAVE; ++w)
        if ((uint32_t)w < wave) wbase += s_wsum[w];
    if (tid < EMIT_SCAN_TILE) s_cum[tid] = wbase + inc - c;
    if (tid == EMIT_SCAN_TILE - 1) s_cum[EMIT_SCAN_TILE] = wbase + inc;
    const int64_t block_out0 = s_red[0] + s_red[1] + s_red[2] + s_red[3];
    __syncthreads();

    int32_t *wstart = s_start + wave * (EMIT_SPW + 1);
    for (uint32_t grp = wave; grp < EMIT_SCAN_TILE / EMIT_SPW; grp += EMIT_WAVES) { // groups of EMIT_SPW positions, one wave each
        const uint32_t j0 = grp * EMIT_SPW;
        if (block_first + j0 >= nv) break; // (wave-uniform)
        const int32_t g0 = s_cum[j0], g1 = s_cum[j0 + EMIT_SPW];
        if (g1 == g0) continue;
        const EmitRec *wrec = s_rec + j0;
        if (lane < EMIT_SPW) wstart[lane] = s_cum[j0 + lane] - g0;
        if (lane == 0) wstart[EMIT_SPW] = g1 - g0;
        __builtin_amdgcn_wave_barrier();
        const int32_t total = g1 - g0;
        const int64_t out0 = block_out0 + g0;
        expand_pairs<MODE>(wrec, wstart, total, out0, tw, isect_ids, keys32, flatten_ids, pos_bits);
        __builtin_amdgcn_wave_barrier(); // the next group reuses wstart
    }
}

// isect_tiles.cu:308-354.  Four consecutive ids per thread (two 16-byte loads + the 8 bytes in front): the kernel streams the
// 8 I bytes of sorted ids once, and the tile arithmetic only runs at the ~T boundaries.
constexpr uint32_t OFFSET_ITEMS = 4;
__global__ void __launch_bounds__(GS_BLOCK) isect_offset_encode_kernel(
    uint32_t n_isects, const int64_t *__restrict__ isect_ids, uint32_t C, uint32_t n_tiles,
    uint32_t tile_n_bits, int32_t *__restrict__ offsets) {
    const uint32_t base = (blockIdx.x * GS_BLOCK + threadIdx.x) * OFFSET_ITEMS;
    if (base >= n_isects) return;
    const int64_t tmask = ((int64_t)1 << tile_n_bits) - 1;
    auto tile_index = [&](int64_t key) { return (key >> tile_n_bits) * (int64_t)n_tiles + (key & tmask); };
    int64_t k[OFFSET_ITEMS];
    if (base + OFFSET_ITEMS <= n_isects && (reinterpret_cast<uintptr_t>(isect_ids) & 15u) == 0u) { // (uniform but for the last thread)
        typedef long long v2ll __attribute__((ext_vector_type(2)));
        const v2ll a = *reinterpret_cast<const v2ll *>(isect_ids + base), b = *reinterpret_cast<const v2ll *>(isect_ids + base + 2);
        k[0] = a.x >> 32; k[1] = a.y >> 32; k[2] = b.x >> 32; k[3] = b.y >> 32;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < OFFSET_ITEMS; ++j) k[j] = base + j < n_isects ? (isect_ids[base + j] >> 32) : 0;
    }
    int64_t prev = base > 0 ? (isect_ids[base - 1] >> 32) : 0;
#pragma unroll
    for (uint32_t j = 0; j < OFFSET_ITEMS; ++j) {
        const uint32_t idx = base + j;
        if (idx >= n_isects) break;
        const int64_t cur = k[j];
        if (idx == 0) {
            const int64_t id_cur = tile_index(cur);
            for (int64_t i = 0; i <= id_cur; ++i) offsets[i] = 0;
        } else if (prev != cur) {
            const int64_t id_prev = tile_index(prev), id_cur = tile_index(cur);
            for (int64_t i = id_prev + 1; i <= id_cur; ++i) offsets[i] = (int32_t)idx;
        }
        if (idx == n_isects - 1) {
            const int64_t id_cur = tile_index(cur);
            for (int64_t i = id_cur + 1; i < (int64_t)C * n_tiles; ++i) offsets[i] = (int32_t)n_isects;
        }
        prev = cur;
    }
}

// ---------------------------------------------------------------------------
// inclusive prefix sum (reduce-then-scan, 3 launches).  2048 items per block.
// ---------------------------------------------------------------------------
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = GS_BLOCK * SCAN_ITEMS;
// scan_apply leaves cum_tiles unwritten from the first scan block that lies entirely behind *n_valid, and an emit wave whose
// first position is valid reads cum_tiles up to its LAST position: an emit wave must never straddle a scan block
static_assert(SCAN_TILE % EMIT_SPW == 0, "GS_EMIT_SPW must divide the scan tile (2048)");

// idx != nullptr: the scanned value is in[idx[i]]; n_valid != nullptr: positions >= *n_valid count as 0
__global__ void __launch_bounds__(GS_BLOCK) scan_block_sums_kernel(
    uint64_t n, const int32_t *__restrict__ in, const int32_t *__restrict__ idx, const uint32_t *__restrict__ n_valid,
    int64_t *__restrict__ block_sums) {
    __shared__ int64_t s_wave[GS_BLOCK / GS_WAVE];
    uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE;
    const uint64_t nv = n_valid != nullptr ? min(n, (uint64_t)*n_valid) : n;
    if (n_valid != nullptr && base >= nv) { // behind the valid prefix: contributes nothing (the spine still sums every block)
        if (threadIdx.x == 0) block_sums[blockIdx.x] = 0;
        return;
    }
    int64_t s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        uint64_t i = base + (uint64_t)k * GS_BLOCK + threadIdx.x;
        if (i < nv) s += idx != nullptr ? in[idx[i]] : in[i];
    }
    const int64_t total = block_scan<GS_BLOCK / GS_WAVE>(s, s_wave).total;
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// single block: in-place exclusive scan of the block sums
__global__ void __launch_bounds__(GS_BLOCK) scan_spine_kernel(uint32_t n_blocks, int64_t *__restrict__ block_sums) {
    __shared__ int64_t s_wave[GS_BLOCK / GS_WAVE];
    int64_t carry = 0;
    for (uint32_t base = 0; base < n_blocks; base += GS_BLOCK) {
        uint32_t i = base + threadIdx.x;
        int64_t v = i < n_blocks ? block_sums[i] : 0;
        const BlockScan<int64_t> sc = block_scan<GS_BLOCK / GS_WAVE>(v, s_wave);
        if (i < n_blocks) block_sums[i] = carry + sc.exc;
        carry += sc.total;
    }
}

template <typename OutT>
__global__ void __launch_bounds__(GS_BLOCK) scan_apply_kernel(
    uint64_t n, const int32_t *__restrict__ in, const int32_t *__restrict__ idx, const uint32_t *__restrict__ n_valid,
    const int64_t *__restrict__ block_sums, OutT *__restrict__ out, int32_t raw_sums) {
    __shared__ int64_t s_wave[GS_BLOCK / GS_WAVE];
    const uint64_t nv = n_valid != nullptr ? min(n, (uint64_t)*n_valid) : n;
    // positions behind the valid prefix carry no element: `out` stays unwritten from the first block that lies entirely
    // behind it (gs_isect_emit* never reads there when it is handed the same n_valid)
    if (n_valid != nullptr && (uint64_t)blockIdx.x * SCAN_TILE >= nv) return;
    // raw_sums: block_sums holds the per-block totals themselves (no spine launch for up to a few thousand blocks):
    // the offset of this block is the sum of its predecessors' totals
    int64_t offset;
    if (raw_sums) {
        int64_t pre = 0;
        for (uint32_t i = threadIdx.x; i < blockIdx.x; i += GS_BLOCK) pre += block_sums[i];
        offset = block_scan<GS_BLOCK / GS_WAVE>(pre, s_wave).total;
    } else {
        offset = block_sums[blockIdx.x];
    }
    // blocked arrangement: thread t owns items [t*ITEMS, (t+1)*ITEMS)
    uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    int32_t v[SCAN_ITEMS];
    int64_t s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        uint64_t i = base + k;
        v[k] = i < nv ? (idx != nullptr ? in[idx[i]] : in[i]) : 0;
        s += v[k];
    }
    int64_t run = block_scan<GS_BLOCK / GS_WAVE>(s, s_wave).exc + offset;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        uint64_t i = base + k;
        run += v[k];
        if (i < n) out[i] = (OutT)run;
    }
}

template <typename OutT>
int32_t cumsum_impl(uint64_t n, const int32_t *in, const int32_t *idx, const uint32_t *n_valid, OutT *out, void *scratch,
                    size_t scratch_bytes, hipStream_t st) {
    if (n == 0) return 0;
    uint32_t n_blocks = gs_div_up(n, SCAN_TILE);
    if (scratch == nullptr || scratch_bytes < (size_t)n_blocks * sizeof(int64_t)) {
        gs_set_error("gs_cumsum: scratch too small (%zu < %zu)", scratch_bytes, (size_t)n_blocks * sizeof(int64_t));
        return 1;
    }
    int64_t *sums = (int64_t *)scratch;
    hipLaunchKernelGGL(scan_block_sums_kernel, dim3(n_blocks), dim3(GS_BLOCK), 0, st, n, in, idx, n_valid, sums);
    const int32_t raw = n_blocks <= 4096u ? 1 : 0; // every block sums its predecessors' totals itself (<= 16 loads per thread)
    if (!raw) hipLaunchKernelGGL(scan_spine_kernel, dim3(1), dim3(GS_BLOCK), 0, st, n_blocks, sums);
    hipLaunchKernelGGL((scan_apply_kernel<OutT>), dim3(n_blocks), dim3(GS_BLOCK), 0, st, n, in, idx, n_valid, sums, out, raw);
    return 0;
}

// ---------------------------------------------------------------------------
// Row binning (see gsplat_hip.h): tile rows by one counting pass over the (splat, row) entries, then every row list expanded
// into its columns.  A "row" is (camera, tile row) = camera * th + y; at most RB_KEYS rows and RB_KEYS columns, one thread each.
// ---------------------------------------------------------------------------
constexpr uint32_t RB_KEYS = 256;              // = GS_ROW_BINNING_MAX_WIDTH = GS_ROW_BINNING_MAX_ROWS = GS_BLOCK
constexpr uint32_t RB_WAVES = GS_BLOCK / GS_WAVE;
constexpr uint32_t RB_POS_ROUNDS = 2;          // positions per thread of a stage-1/3 block
constexpr uint32_t RB_POS_ITEMS = GS_BLOCK * RB_POS_ROUNDS;
constexpr uint32_t RB_ROUNDS = 2;              // entries per thread of a chunk
constexpr uint32_t RB_ITEMS = GS_BLOCK * RB_ROUNDS; // entries per chunk of a row list
constexpr uint32_t RB_STAGE_CAP = 4096;        // pairs of a chunk the expansion can stage in LDS (mean 3.2 per entry on a 1080p frame)
static_assert(RB_KEYS == GS_BLOCK && GS_ROW_BINNING_MAX_WIDTH == RB_KEYS && GS_ROW_BINNING_MAX_ROWS == RB_KEYS, "one thread per row / column");
static_assert(GS_ROW_BINNING_MAX_WIDTH < (1u << 16), "x0 | x1 << 16 in one word");

struct RbItem {
    int32_t row0, row1, x0, x1; // rows [row0, row1), columns [x0, x1); empty: row0 == row1
};

// the splat at position `pos` of the depth order (pos < nv), as isect_emit_scan_kernel gathers it
GS_DEV RbItem rb_item(uint32_t pos, uint32_t nv, uint32_t N, uint32_t C, const int32_t *__restrict__ perm, const float *__restrict__ means2d,
                      uint32_t s_m2, const int32_t *__restrict__ radii, float tile_size, int32_t tw, int32_t th) {
    RbItem it = {0, 0, 0, 0};
    if (pos >= nv) return it;
    const uint32_t e = (uint32_t)perm[pos];
    const int32_t r = radii[e];
    if (r <= 0) return it;
    const float2 m = *reinterpret_cast<const float2 *>(means2d + (size_t)e * s_m2);
    const TileBox b = tile_box(m.x, m.y, r, tile_size, tw, th);
    const uint32_t cid = e / N;
    if (b.x1 <= b.x0 || b.y1 <= b.y0 || cid >= C) return it;
    it.row0 = (int32_t)cid * th + b.y0;
    it.row1 = (int32_t)cid * th + b.y1;
    it.x0 = b.x0;
    it.x1 = b.x1;
    return it;
}

GS_DEV uint32_t rb_nv(uint32_t n_elems, uint32_t n_kept, const uint32_t *__restrict__ n_valid) {
    const uint32_t nv = min(n_elems, n_kept);
    return n_valid != nullptr ? min(nv, *n_valid) : nv;
}

// Stage 1: per block of RB_ITEMS positions, the number of splats that cover each row and the pairs they have there
// (difference arrays in LDS: integer sums, their order does not matter).  row_cnt / row_pairs: [rows][n_blocks].
__global__ void __launch_bounds__(GS_BLOCK) rb_row_hist_kernel(
    uint32_t n_elems, uint32_t n_kept, uint32_t N, uint32_t C, const int32_t *__restrict__ perm, const uint32_t *__restrict__ n_valid,
    const float *__restrict__ means2d, uint32_t s_m2, const int32_t *__restrict__ radii, float tile_size, int32_t tw, int32_t th,
    uint32_t rows, uint32_t n_blocks, uint32_t *__restrict__ row_cnt, uint32_t *__restrict__ row_pairs, uint2 *__restrict__ items) {
    __shared__ int32_t s_cnt[RB_KEYS + 1], s_pairs[RB_KEYS + 1], s_w[RB_WAVES];
    const uint32_t tid = threadIdx.x;
    s_cnt[tid] = 0;
    s_pairs[tid] = 0;
    if (tid == 0) s_cnt[RB_KEYS] = s_pairs[RB_KEYS] = 0;
    __syncthreads();
    const uint32_t nv = rb_nv(n_elems, n_kept, n_valid);
    RbItem its[RB_POS_ROUNDS]; // (all gathers of the thread in flight together)
#pragma unroll
    for (uint32_t k = 0; k < RB_POS_ROUNDS; ++k)
        its[k] = rb_item(blockIdx.x * RB_POS_ITEMS + k * GS_BLOCK + tid, nv, N, C, perm, means2d, s_m2, radii, tile_size, tw, th);
#pragma unroll
    for (uint32_t k = 0; k < RB_POS_ROUNDS; ++k) {
        const RbItem it = its[k];
        // the item, for stage 3 (rows | columns, 16 bits each): the gathers through perm happen once
        const uint32_t pos = blockIdx.x * RB_POS_ITEMS + k * GS_BLOCK + tid;
        if (pos < nv) items[pos] = make_uint2((uint32_t)it.row0 | ((uint32_t)it.row1 << 16), (uint32_t)it.x0 | ((uint32_t)it.x1 << 16));
        if (it.row1 > it.row0) {
            const int32_t w = it.x1 - it.x0;
            atomicAdd(&s_cnt[it.row0], 1);
            atomicAdd(&s_cnt[it.row1], -1);
            atomicAdd(&s_pairs[it.row0], w);
            atomicAdd(&s_pairs[it.row1], -w);
        }
    }
    __syncthreads();
    const int32_t c = block_scan<RB_WAVES>(s_cnt[tid], s_w).inc;
    const int32_t p = block_scan<RB_WAVES>(s_pairs[tid], s_w).inc;
    if (tid < rows) {
        row_cnt[(size_t)tid * n_blocks + blockIdx.x] = (uint32_t)c;
        row_pairs[(size_t)tid * n_blocks + blockIdx.x] = (uint32_t)p;
    }
}

// Stage 2 (one workgroup per row): exclusive scan of the row's counts over the blocks, in place -- the place of every block's
// first entry inside the row's list -- and the row's totals: row_total[r] entries, row_total[rows + r] pairs.
__global__ void __launch_bounds__(GS_BLOCK) rb_row_scan_kernel(
    uint32_t rows, uint32_t n_blocks, uint32_t *__restrict__ row_cnt, const uint32_t *__restrict__ row_pairs,
    uint32_t *__restrict__ row_total, uint32_t tw, int32_t *__restrict__ tile_total) {
    __shared__ int32_t s_w[RB_WAVES];
    const uint32_t tid = threadIdx.x, r = blockIdx.x;
    if (tid < tw) tile_total[(size_t)r * tw + tid] = 0; // stage 4 adds the chunks' column counts up here (the offsets array)
    uint32_t *cnt = row_cnt + (size_t)r * n_blocks;
    const uint32_t *pairs = row_pairs + (size_t)r * n_blocks;
    uint32_t carry = 0, psum = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += GS_BLOCK) {
        const uint32_t b = b0 + tid;
        const uint32_t c = b < n_blocks ? cnt[b] : 0u;
        psum += b < n_blocks ? pairs[b] : 0u;
        const BlockScan<int32_t> sc = block_scan<RB_WAVES>((int32_t)c, s_w);
        if (b < n_blocks) cnt[b] = carry + (uint32_t)sc.exc;
        carry += (uint32_t)sc.total;
    }
    const uint32_t ptot = (uint32_t)block_scan<RB_WAVES>((int32_t)psum, s_w).total;
    if (tid == 0) {
        row_total[r] = carry;
        row_total[rows + r] = ptot;
    }
}

// rb_row_scatter_kernel's scan (through rb_row_tables), kept as the parent commit had it: with block_scan the kernel measured
// 9.90 us against the parent's 9.77 us at config 2, over the bar of parent mean + spread (9.85 us; six alternating pairs,
// profiles/binning_shared_stages_ab.txt).  Inclusive scan of one int per thread over the workgroup; s_w: WAVES ints, free again on return.
template <uint32_t WAVES>
GS_DEV int32_t rb_block_inclusive_scan(int32_t v, int32_t *s_w) {
    const uint32_t lane = threadIdx.x % GS_WAVE, wave = threadIdx.x / GS_WAVE;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int32_t o = __shfl_up(v, off, 64);
        if (lane >= (uint32_t)off) v += o;
    }
    if (lane == GS_WAVE - 1) s_w[wave] = v;
    __syncthreads();
    int32_t base = 0;
#pragma unroll
    for (uint32_t w = 0; w < WAVES; ++w)
        if (w < wave) base += s_w[w];
    __syncthreads();
    return base + v;
}

// What the later stages need of the rows, from row_total, by every workgroup for itself (rows <= 256 values, one scan each):
// s_rs[r] = where list r begins (s_rs[rows] = all entries); s_cf[r] = number of chunks (RB_ITEMS entries, never across two
// rows) in front of row r.  Both hold rows + 1 values.  Returns the pairs of the rows in front of row `tid` (0 from `rows` on).
GS_DEV uint32_t rb_row_tables(uint32_t rows, const uint32_t *__restrict__ row_total, uint32_t *s_rs, uint32_t *s_cf, int32_t *s_w) {
    const uint32_t tid = threadIdx.x;
    const uint32_t len = tid < rows ? row_total[tid] : 0u, pairs = tid < rows ? row_total[rows + tid] : 0u;
    const uint32_t nc = (len + RB_ITEMS - 1) / RB_ITEMS;
    const uint32_t rs = (uint32_t)rb_block_inclusive_scan<RB_WAVES>((int32_t)len, s_w);
    const uint32_t cf = (uint32_t)rb_block_inclusive_scan<RB_WAVES>((int32_t)nc, s_w);
    const uint32_t pb = (uint32_t)rb_block_inclusive_scan<RB_WAVES>((int32_t)pairs, s_w);
    s_rs[tid] = rs - len;
    s_cf[tid] = cf - nc;
    if (tid == GS_BLOCK - 1) {
        s_rs[RB_KEYS] = rs;
        s_cf[RB_KEYS] = cf;
    }
    __syncthreads();
    return pb - pairs;
}

// the same tables as stage 3's first workgroup left them in memory (stages 4 to 6); ends with a barrier
GS_DEV void rb_load_tables(uint32_t rows, const uint32_t *__restrict__ tables, uint32_t *s_rs, uint32_t *s_cf) {
    for (uint32_t i = threadIdx.x; i <= rows; i += GS_BLOCK) {
        s_rs[i] = tables[i];
        s_cf[i] = tables[(rows + 1) + i];
    }
    __syncthreads();
}

// Rank of every item among the EARLIER items of the workgroup's list that cover the same key (row or column), for every key
// in the item's range [lo, hi).  Thread t holds the items k * GS_BLOCK + t of the list, k < R; R * 4 wave slots in list order.
// The lanes of a slot OR their lane bit into one 64-bit mask per key; rank = the bits below the lane's own + the counts of
// the earlier slots (s_sbase) -- a function of the list order alone.  rb_rank_prepare builds masks and slot bases and returns
// the list's number of items that cover key `tid`; all threads of the workgroup call it together, and a barrier has to follow
// before rb_rank_of is used (and another before the next call).
template <uint32_t R>
GS_DEV uint32_t rb_rank_prepare(const int32_t (&lo)[R], const int32_t (&hi)[R], uint32_t n_keys, unsigned long long (*s_mask)[RB_KEYS],
                                uint32_t (*s_sbase)[RB_KEYS]) {
    const uint32_t tid = threadIdx.x, lane = tid % GS_WAVE, wave = tid / GS_WAVE;
#pragma unroll
    for (uint32_t s = 0; s < R * RB_WAVES; ++s) s_mask[s][tid] = 0ull;
    __syncthreads();
    const unsigned long long bit = 1ull << lane;
#pragma unroll
    for (uint32_t k = 0; k < R; ++k)
        for (int32_t key = lo[k]; key < hi[k]; ++key) atomicOr(&s_mask[k * RB_WAVES + wave][key], bit);
    __syncthreads();
    uint32_t b = 0;
    if (tid < n_keys) {
#pragma unroll
        for (uint32_t s = 0; s < R * RB_WAVES; ++s) {
            s_sbase[s][tid] = b;
            b += (uint32_t)__popcll(s_mask[s][tid]);
        }
    }
    return b;
}
GS_DEV uint32_t rb_rank_of(uint32_t k, int32_t key, const unsigned long long (*s_mask)[RB_KEYS], const uint32_t (*s_sbase)[RB_KEYS]) {
    const uint32_t lane = threadIdx.x % GS_WAVE, s = k * RB_WAVES + threadIdx.x / GS_WAVE;
    return s_sbase[s][key] + (uint32_t)__popcll(s_mask[s][key] & ((1ull << lane) - 1ull));
}

// Stage 3: one 8-byte entry (position, x0 | x1 << 16) per splat and covered row, into that row's list in position order.
__global__ void __launch_bounds__(GS_BLOCK) rb_row_scatter_kernel(
    uint32_t n_elems, uint32_t n_kept, const uint32_t *__restrict__ n_valid, const uint2 *__restrict__ items, uint32_t rows, uint32_t n_blocks,
    const uint32_t *__restrict__ row_base, const uint32_t *__restrict__ row_total, uint32_t *__restrict__ tables, uint2 *__restrict__ entries,
    uint32_t capacity) {
    __shared__ unsigned long long s_mask[RB_POS_ROUNDS * RB_WAVES][RB_KEYS];
    __shared__ uint32_t s_sbase[RB_POS_ROUNDS * RB_WAVES][RB_KEYS];
    __shared__ uint32_t s_gbase[RB_KEYS], s_rs[RB_KEYS + 1], s_cf[RB_KEYS + 1];
    __shared__ int32_t s_w[RB_WAVES];
    const uint32_t tid = threadIdx.x;
    const uint32_t nv = rb_nv(n_elems, n_kept, n_valid);
    int32_t lo[RB_POS_ROUNDS], hi[RB_POS_ROUNDS];
    uint2 ent[RB_POS_ROUNDS];
#pragma unroll
    for (uint32_t k = 0; k < RB_POS_ROUNDS; ++k) {
        const uint32_t pos = blockIdx.x * RB_POS_ITEMS + k * GS_BLOCK + tid;
        const uint2 it = pos < nv ? items[pos] : make_uint2(0u, 0u);
        lo[k] = (int32_t)min(it.x & 0xffffu, rows);
        hi[k] = (int32_t)min(it.x >> 16, rows);
        ent[k] = make_uint2(pos, it.y);
    }
    const uint32_t pb = rb_row_tables(rows, row_total, s_rs, s_cf, s_w);
    if (blockIdx.x == 0) { // the same in every workgroup: the first one leaves them for stages 4 to 6 (row_start | chunk_first | pairs_before)
        for (uint32_t i = tid; i <= rows; i += GS_BLOCK) {
            tables[i] = s_rs[i];
            tables[(rows + 1) + i] = s_cf[i];
        }
        if (tid < rows) tables[2 * (rows + 1) + tid] = pb;
    }
    s_gbase[tid] = tid < rows ? s_rs[tid] + row_base[(size_t)tid * n_blocks + blockIdx.x] : 0u;
    rb_rank_prepare<RB_POS_ROUNDS>(lo, hi, rows, s_mask, s_sbase);
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < RB_POS_ROUNDS; ++k)
        for (int32_t row = lo[k]; row < hi[k]; ++row) {
            const uint32_t place = s_gbase[row] + rb_rank_of(k, row, s_mask, s_sbase);
            if (place < capacity) entries[place] = ent[k];
        }
}

// chunk -> (row, entry range).  s_cf / s_rs: chunk_first / row_start in LDS (rows + 1 values each).
GS_DEV uint32_t rb_chunk_row(uint32_t chunk, uint32_t rows, const uint32_t *s_cf) {
    uint32_t r = 0; // largest r with chunk_first[r] <= chunk (rows without entries share their successor's value and are skipped)
#pragma unroll
    for (uint32_t step = RB_KEYS / 2; step > 0; step >>= 1)
        if (r + step < rows && s_cf[r + step] <= chunk) r += step;
    return r;
}

// Stage 4: per chunk of a row list, the number of its entries that cover each column.  col_cnt: [chunks][tw].
__global__ void __launch_bounds__(GS_BLOCK) rb_col_hist_kernel(
    uint32_t rows, uint32_t tw, const uint32_t *__restrict__ tables, const uint2 *__restrict__ entries, uint32_t capacity,
    uint32_t max_chunks, uint32_t *__restrict__ col_cnt, int32_t *__restrict__ tile_total) {
    __shared__ uint32_t s_cf[RB_KEYS + 1], s_rs[RB_KEYS + 1];
    __shared__ int32_t s_diff[RB_KEYS + 1], s_w[RB_WAVES];
    const uint32_t tid = threadIdx.x;
    rb_load_tables(rows, tables, s_rs, s_cf);
    const uint32_t n_chunks = min(s_cf[rows], max_chunks);
    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint32_t r = rb_chunk_row(chunk, rows, s_cf);
        const uint32_t start = s_rs[r] + (chunk - s_cf[r]) * RB_ITEMS, end = min(min(start + RB_ITEMS, s_rs[r + 1]), capacity);
        s_diff[tid] = 0;
        if (tid == 0) s_diff[RB_KEYS] = 0;
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < RB_ROUNDS; ++k) {
            const uint32_t i = start + k * GS_BLOCK + tid;
            if (i < end) {
                const uint32_t xx = entries[i].y;
                atomicAdd(&s_diff[min(xx & 0xffffu, RB_KEYS)], 1);
                atomicAdd(&s_diff[min(xx >> 16, RB_KEYS)], -1);
            }
        }
        __syncthreads();
        const int32_t c = block_scan<RB_WAVES>(s_diff[tid], s_w).inc;
        if (tid < tw) {
            col_cnt[(size_t)chunk * tw + tid] = (uint32_t)c;
            if (c != 0) atomicAdd(&tile_total[(size_t)r * tw + tid], c); // (an integer sum: the same whatever the order)
        }
    }
}

// Stage 5, two kinds of workgroups in one launch.  Workgroup r < rows: offsets[tile] of row r from the tile totals stage 4
// left there = pairs of the rows in front + pairs of the row's tiles in front -- every tile is written, the empty ones too.
// The others: one wave per tile, the exclusive scan of the tile's counts over its row's chunks, in place (64 chunks a step).
__global__ void __launch_bounds__(GS_BLOCK) rb_col_scan_kernel(
    uint32_t rows, uint32_t tw, const uint32_t *__restrict__ tables, uint32_t max_chunks, uint32_t *__restrict__ col_cnt,
    int32_t *__restrict__ offsets) {
    __shared__ int32_t s_w[RB_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid % GS_WAVE;
    if (blockIdx.x < rows) { // (block-uniform)
        const uint32_t r = blockIdx.x;
        const uint32_t tot = tid < tw ? (uint32_t)offsets[(size_t)r * tw + tid] : 0u;
        const uint32_t inc = (uint32_t)block_scan<RB_WAVES>((int32_t)tot, s_w).inc;
        if (tid < tw) offsets[(size_t)r * tw + tid] = (int32_t)(tables[2 * (rows + 1) + r] + inc - tot);
        return;
    }
    const uint32_t task = (blockIdx.x - rows) * RB_WAVES + tid / GS_WAVE;
    if (task >= rows * tw) return; // (wave-uniform; no barrier below)
    const uint32_t r = task / tw, x = task - r * tw;
    const uint32_t c0 = min(tables[(rows + 1) + r], max_chunks), c1 = min(tables[(rows + 1) + r + 1], max_chunks);
    uint32_t carry = 0;
    for (uint32_t cb = c0; cb < c1; cb += GS_WAVE) {
        const uint32_t c = cb + lane;
        uint32_t *p = col_cnt + (size_t)c * tw + x;
        const uint32_t v = c < c1 ? *p : 0u;
        const uint32_t inc = wave_inclusive_scan(v);
        if (c < c1) *p = carry + inc - v;
        carry += __shfl(inc, GS_WAVE - 1, 64);
    }
}

// Stage 6: every chunk writes, for each of its entries and each column the entry covers, the pair's id and flatten id at
// offsets[tile] + the chunk's base in the tile + the entry's rank among the chunk's earlier entries that cover the column.
// The pairs of a chunk in one tile are neighbours in the output: they are first put in output order in LDS (column | entry,
// 4 bytes a pair) and written from there, consecutive lanes to consecutive places; a chunk with more than RB_STAGE_CAP pairs
// writes every pair straight from its entry's lane.
__global__ void __launch_bounds__(GS_BLOCK) rb_expand_kernel(
    uint32_t n_elems, uint32_t rows, uint32_t tw, uint32_t th, uint32_t tile_n_bits, const uint32_t *__restrict__ tables,
    const uint2 *__restrict__ entries, uint32_t capacity, uint32_t max_chunks, const uint32_t *__restrict__ col_base,
    const int32_t *__restrict__ offsets, const int32_t *__restrict__ perm, const uint64_t *__restrict__ sorted_keys,
    const float *__restrict__ depths, uint32_t n_isects, int64_t *__restrict__ isect_ids, int32_t *__restrict__ flatten_ids) {
    __shared__ unsigned long long s_mask[RB_ROUNDS * RB_WAVES][RB_KEYS];
    __shared__ uint32_t s_sbase[RB_ROUNDS * RB_WAVES][RB_KEYS];
    __shared__ uint32_t s_gbase[RB_KEYS], s_colpre[RB_KEYS + 1], s_cf[RB_KEYS + 1], s_rs[RB_KEYS + 1];
    __shared__ uint32_t s_stage[RB_STAGE_CAP];
    __shared__ int32_t s_v[RB_ITEMS], s_db[RB_ITEMS];
    __shared__ int32_t s_w[RB_WAVES];
    const uint32_t tid = threadIdx.x;
    rb_load_tables(rows, tables, s_rs, s_cf);
    const uint32_t n_chunks = min(s_cf[rows], max_chunks);
    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint32_t r = rb_chunk_row(chunk, rows, s_cf);
        const uint32_t start = s_rs[r] + (chunk - s_cf[r]) * RB_ITEMS, end = min(min(start + RB_ITEMS, s_rs[r + 1]), capacity);
        const uint32_t cid = r / th, y = r - cid * th;
        const uint32_t key_row = (cid << tile_n_bits) | (y * tw); // + column = the pair's 32-bit key
        if (tid < tw) s_gbase[tid] = (uint32_t)offsets[(size_t)r * tw + tid] + col_base[(size_t)chunk * tw + tid];
        int32_t lo[RB_ROUNDS], hi[RB_ROUNDS], v[RB_ROUNDS], db[RB_ROUNDS];
        uint2 ent[RB_ROUNDS];
#pragma unroll
        for (uint32_t k = 0; k < RB_ROUNDS; ++k) {
            const uint32_t i = start + k * GS_BLOCK + tid;
            ent[k] = i < end ? entries[i] : make_uint2(0u, 0u);
            if (ent[k].x >= n_elems) ent[k] = make_uint2(0u, 0u); // (never: positions come from stage 3; keeps the gathers in bounds)
        }
#pragma unroll
        for (uint32_t k = 0; k < RB_ROUNDS; ++k) {
            lo[k] = (int32_t)min(ent[k].y & 0xffffu, tw);
            hi[k] = (int32_t)min(ent[k].y >> 16, tw);
            v[k] = 0;
            db[k] = 0;
            if (hi[k] > lo[k]) pair_id_of(ent[k].x, sorted_keys, perm, depths, &v[k], &db[k]);
            s_v[k * GS_BLOCK + tid] = v[k];
            s_db[k * GS_BLOCK + tid] = db[k];
        }
        const uint32_t cnt = rb_rank_prepare<RB_ROUNDS>(lo, hi, tw, s_mask, s_sbase);
        const uint32_t inc = (uint32_t)block_scan<RB_WAVES>((int32_t)cnt, s_w).inc; // (cnt is 0 from column tw on)
        s_colpre[tid] = inc - cnt;
        if (tid == GS_BLOCK - 1) s_colpre[RB_KEYS] = inc;
        __syncthreads();
        const uint32_t total = s_colpre[RB_KEYS];
        // the id as the other routes form it: key << 32 | the depth's bits, sign-extended (isect_tiles.cu:91)
        if (total <= RB_STAGE_CAP) { // (block-uniform)
#pragma unroll
            for (uint32_t k = 0; k < RB_ROUNDS; ++k)
                for (int32_t x = lo[k]; x < hi[k]; ++x) {
                    const uint32_t at = s_colpre[x] + rb_rank_of(k, x, s_mask, s_sbase);
                    if (at < RB_STAGE_CAP) s_stage[at] = ((uint32_t)x << 16) | (k * GS_BLOCK + tid);
                }
            __syncthreads();
            for (uint32_t i = tid; i < total; i += GS_BLOCK) {
                const uint32_t w = s_stage[i], x = w >> 16, e = w & 0xffffu;
                const uint32_t place = s_gbase[x] + (i - s_colpre[x]);
                if (place < n_isects) {
                    isect_ids[place] = (int64_t)((uint64_t)(key_row + x) << 32) | (int64_t)s_db[e];
                    flatten_ids[place] = s_v[e];
                }
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < RB_ROUNDS; ++k)
                for (int32_t x = lo[k]; x < hi[k]; ++x) {
                    const uint32_t place = s_gbase[x] + rb_rank_of(k, x, s_mask, s_sbase);
                    if (place < n_isects) {
                        isect_ids[place] = (int64_t)((uint64_t)(key_row + (uint32_t)x) << 32) | (int64_t)db[k];
                        flatten_ids[place] = v[k];
                    }
                }
        }
        __syncthreads(); // the next chunk sets the tables and clears the masks
    }
}

} // namespace

extern "C" int32_t gs_isect_count(
    uint32_t n_elems, const float *means2d, uint32_t means2d_stride, const int32_t *radii, uint32_t tile_size,
    uint32_t tile_width, uint32_t tile_height, int32_t *tiles_per_gauss, gs_stream_t stream) {
    if (n_elems == 0) return 0;
    GS_CHECK_ARG(means2d && radii && tiles_per_gauss, "null pointer");
    GS_CHECK_ARG(tile_size > 0, "tile_size must be > 0");
    GS_CHECK_ARG(means2d_stride >= 2 && means2d_stride % 2 == 0, "means2d_stride must be even and >= 2");
    hipLaunchKernelGGL(isect_count_kernel, dim3(gs_div_up(n_elems, GS_BLOCK)), dim3(GS_BLOCK), 0,
                       (hipStream_t)stream, n_elems, means2d, means2d_stride, radii, (float)tile_size, (int32_t)tile_width,
                       (int32_t)tile_height, tiles_per_gauss);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t gs_cumsum_scratch_bytes(uint64_t n) {
    return (size_t)(gs_div_up(n, SCAN_TILE) + 1) * sizeof(int64_t);
}

extern "C" int32_t gs_cumsum_i32(
    uint64_t n, const int32_t *in, int64_t *out, void *scratch, size_t scratch_bytes, gs_stream_t stream) {
    if (n == 0) return 0;
    GS_CHECK_ARG(in && out, "null pointer");
    int32_t rc = cumsum_impl<int64_t>(n, in, nullptr, nullptr, out, scratch, scratch_bytes, (hipStream_t)stream);
    if (rc) return rc;
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_cumsum_i32_i32(
    uint64_t n, const int32_t *in, int32_t *out, void *scratch, size_t scratch_bytes, gs_stream_t stream) {
    if (n == 0) return 0;
    GS_CHECK_ARG(in && out, "null pointer");
    int32_t rc = cumsum_impl<int32_t>(n, in, nullptr, nullptr, out, scratch, scratch_bytes, (hipStream_t)stream);
    if (rc) return rc;
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_cumsum_gather_i32(
    uint64_t n, const int32_t *in, const int32_t *idx, const uint32_t *n_valid, int64_t *out, void *scratch,
    size_t scratch_bytes, gs_stream_t stream) {
    if (n == 0) return 0;
    GS_CHECK_ARG(in && idx && out, "null pointer");
    int32_t rc = cumsum_impl<int64_t>(n, in, idx, n_valid, out, scratch, scratch_bytes, (hipStream_t)stream);
    if (rc) return rc;
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" uint32_t gs_isect_count_blocks(uint32_t n_elems) { return gs_div_up(n_elems, GS_BLOCK * COUNT_ITEMS); }

extern "C" int32_t gs_isect_count_keys(
    uint32_t n_elems, const float *means2d, uint32_t means2d_stride, const int32_t *radii, const float *depths, uint32_t tile_size,
    uint32_t tile_width, uint32_t tile_height, int32_t *tiles_per_gauss, int64_t *keys, int32_t *vals, int32_t *block_sums,
    void *sort_temp, size_t sort_temp_bytes, const int64_t *bucket_splitters, gs_stream_t stream) {
    if (n_elems == 0) return 0;
    GS_CHECK_ARG(radii && depths && tiles_per_gauss && keys && (vals || bucket_splitters), "null pointer (vals may be NULL with bucket_splitters only)");
    GS_CHECK_ARG(means2d != nullptr || block_sums == nullptr, "means2d NULL (tiles_per_gauss given): the block sums were made with the counts");
    GS_CHECK_ARG(bucket_splitters == nullptr || sort_temp != nullptr, "bucket_splitters come with sort_temp (the histogram's place)");
    GS_CHECK_ARG(tile_size > 0, "tile_size must be > 0");
    GS_CHECK_ARG(means2d_stride >= 2 && means2d_stride % 2 == 0, "means2d_stride must be even and >= 2");
    uint32_t n_blocks = 0;
    uint32_t *hist = nullptr;
    if (sort_temp != nullptr) {
        hist = sort_first_hist_slot(n_elems, sort_temp, sort_temp_bytes, &n_blocks);
        GS_CHECK_ARG(hist != nullptr && n_blocks == gs_isect_count_blocks(n_elems),
                     "sort_temp given, but gs_sort_first_hist_applicable(n_elems) is 0 or the buffer is too small");
    }
    hipLaunchKernelGGL(isect_count_keys_kernel, dim3(gs_isect_count_blocks(n_elems)), dim3(GS_BLOCK), 0, (hipStream_t)stream,
                       n_elems, means2d, means2d_stride, radii, depths, (float)tile_size, (int32_t)tile_width, (int32_t)tile_height,
                       tiles_per_gauss, keys, vals, block_sums, hist, n_blocks, (const uint64_t *)bucket_splitters);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_isect_depth_keys(
    uint32_t n_elems, const int32_t *radii, const float *depths, int64_t *keys, int32_t *vals, gs_stream_t stream) {
    if (n_elems == 0) return 0;
    GS_CHECK_ARG(radii && depths && keys && vals, "null pointer");
    hipLaunchKernelGGL(isect_depth_keys_kernel, dim3(gs_div_up(n_elems, GS_BLOCK)), dim3(GS_BLOCK), 0,
                       (hipStream_t)stream, n_elems, radii, depths, keys, vals);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_gather_i32(uint32_t n, const int32_t *src, const int32_t *idx, int32_t *out, gs_stream_t stream) {
    if (n == 0) return 0;
    GS_CHECK_ARG(src && idx && out, "null pointer");
    hipLaunchKernelGGL(gather_i32_kernel, dim3(gs_div_up(n, GS_BLOCK)), dim3(GS_BLOCK), 0, (hipStream_t)stream, n, src, idx, out);
    GS_CHECK_LAUNCH();
    return 0;
}

// The argument checks the emission entry points share.  `who` is the name the error text carries (GS_CHECK_ARG would print
// this function's); ptr_msg: the entry point's own pointer check, NULL when it passed.
static int32_t emit_check_args(const char *who, const char *ptr_msg, const int64_t *camera_ids, uint32_t N, uint32_t tile_n_bits,
                               uint32_t means2d_stride, uint32_t tile_width, uint32_t tile_height) {
    const char *msg = ptr_msg != nullptr                               ? ptr_msg
                      : !(camera_ids != nullptr || N > 0)              ? "N must be > 0 when camera_ids is NULL"
                      : !(tile_n_bits < 32)                            ? "tile_n_bits must be < 32"
                      : !(means2d_stride >= 2 && means2d_stride % 2 == 0) ? "means2d_stride must be even and >= 2"
                      // expand_pairs divides a pair's offset inside its splat's box (< tiles of the grid) in float arithmetic
                      : !((uint64_t)tile_width * tile_height <= (1ull << 24)) ? "the tile grid must have at most 2^24 tiles"
                                                                       : nullptr;
    if (msg == nullptr) return 0;
    gs_set_error("%s: %s", who, msg);
    return 1;
}

template <bool COMPACT>
static int32_t emit_launch(
    const char *who, const char *ptr_msg, uint32_t n_elems, uint32_t N, const int32_t *perm, const uint32_t *n_valid,
    const int64_t *camera_ids, const float *means2d, uint32_t means2d_stride, const int32_t *radii, const float *depths,
    const int64_t *cum_tiles_per_gauss, uint32_t tile_size, uint32_t tile_width, uint32_t tile_height, uint32_t tile_n_bits,
    int64_t *isect_ids, uint32_t *keys32, int32_t *flatten_ids, gs_stream_t stream) {
    if (emit_check_args(who, ptr_msg, camera_ids, N, tile_n_bits, means2d_stride, tile_width, tile_height)) return 1;
    hipLaunchKernelGGL(isect_emit_kernel<COMPACT>, dim3(gs_div_up(n_elems, EMIT_WAVES * EMIT_SPW)), dim3(GS_BLOCK), 0,
                       (hipStream_t)stream, n_elems, N, perm, n_valid, camera_ids, means2d, means2d_stride, radii, depths,
                       cum_tiles_per_gauss, (float)tile_size, (int32_t)tile_width, (int32_t)tile_height,
                       tile_n_bits, isect_ids, keys32, flatten_ids);
    return 0;
}

extern "C" int32_t gs_isect_emit(
    uint32_t n_elems, uint32_t N, const int32_t *perm, const uint32_t *n_valid, const int64_t *camera_ids, const float *means2d,
    uint32_t means2d_stride, const int32_t *radii, const float *depths, const int64_t *cum_tiles_per_gauss,
    uint32_t tile_size, uint32_t tile_width, uint32_t tile_height, uint32_t tile_n_bits,
    int64_t *isect_ids, int32_t *flatten_ids, gs_stream_t stream) {
    if (n_elems == 0) return 0;
    const bool ptrs = means2d && radii && depths && cum_tiles_per_gauss;
    if (int32_t rc = emit_launch<false>(__func__, ptrs ? nullptr : "null pointer", n_elems, N, perm, n_valid, camera_ids, means2d,
                                        means2d_stride, radii, depths, cum_tiles_per_gauss, tile_size, tile_width, tile_height,
                                        tile_n_bits, isect_ids, nullptr, flatten_ids, stream))
        return rc;
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_isect_emit_compact(
    uint32_t n_elems, uint32_t N, const int32_t *perm, const uint32_t *n_valid, const int64_t *camera_ids, const float *means2d,
    uint32_t means2d_stride, const int32_t *radii, const float *depths, const int64_t *cum_tiles_per_gauss,
    uint32_t tile_size, uint32_t tile_width, uint32_t tile_height, uint32_t tile_n_bits,
    uint32_t *keys32, int32_t *flatten_ids, gs_stream_t stream) {
    if (n_elems == 0) return 0;
    const bool ptrs = means2d && radii && depths && cum_tiles_per_gauss && keys32 && flatten_ids;
    if (int32_t rc = emit_launch<true>(__func__, ptrs ? nullptr : "null pointer", n_elems, N, perm, n_valid, camera_ids, means2d,
                                       means2d_stride, radii, depths, cum_tiles_per_gauss, tile_size, tile_width, tile_height,
                                       tile_n_bits, nullptr, keys32, flatten_ids, stream))
        return rc;
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" uint32_t gs_isect_emit_group_shift(void) { return EMIT_SCAN_SHIFT; }
// Above this many groups the emission wants the groups' prefix sum (group_prefix): without it every workgroup adds up its
// predecessors' sums itself, a number of loads quadratic in the number of groups (fine for a 1 M-element frame: 7.9 K groups).
extern "C" uint32_t gs_isect_emit_prefix_from_groups(void) { return 8192u; }

// mode 0 / 1 / 2: see isect_emit_scan_kernel
static int32_t emit_presorted_launch(
    int mode, uint32_t pos_bits, uint32_t n_elems, uint32_t N, const int32_t *perm, const uint32_t *n_valid, const int64_t *camera_ids,
    const float *means2d, uint32_t means2d_stride, const int32_t *radii, const float *depths, const int32_t *tiles_per_gauss,
    const uint32_t *group_sums, const int64_t *group_prefix, uint32_t tile_size, uint32_t tile_width, uint32_t tile_height,
    uint32_t tile_n_bits, int64_t *isect_ids, uint32_t *keys32, int32_t *flatten_ids, gs_stream_t stream) {
    if (n_elems == 0) return 0;
    const char *ptr_msg = !(means2d && radii && depths && tiles_per_gauss && (group_sums || group_prefix) && (flatten_ids || mode == 2)) ? "null pointer"
                          : !(mode != 0 ? keys32 != nullptr : isect_ids != nullptr)                                                    ? "null output"
                                                                                                                                        : nullptr;
    if (emit_check_args(__func__, ptr_msg, camera_ids, N, tile_n_bits, means2d_stride, tile_width, tile_height)) return 1;
    GS_CHECK_ARG(n_elems < (1u << 31), "n_elems must be < 2^31");
    // (a mode's kernel never touches the outputs of the other modes)
    const auto kernel = mode == 2 ? isect_emit_scan_kernel<2> : mode == 1 ? isect_emit_scan_kernel<1> : isect_emit_scan_kernel<0>;
    hipLaunchKernelGGL(kernel, dim3(gs_div_up(n_elems, EMIT_SCAN_TILE)), dim3(GS_BLOCK), 0, (hipStream_t)stream, n_elems, N, perm, n_valid,
                       camera_ids, means2d, means2d_stride, radii, depths, tiles_per_gauss, group_sums, group_prefix, (float)tile_size,
                       (int32_t)tile_width, (int32_t)tile_height, tile_n_bits, isect_ids, keys32, flatten_ids, pos_bits);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_isect_emit_presorted(
    uint32_t n_elems, uint32_t N, const int32_t *perm, const uint32_t *n_valid, const int64_t *camera_ids, const float *means2d,
    uint32_t means2d_stride, const int32_t *radii, const float *depths, const int32_t *tiles_per_gauss, const uint32_t *group_sums,
    const int64_t *group_prefix, uint32_t tile_size, uint32_t tile_width, uint32_t tile_height, uint32_t tile_n_bits, int32_t compact,
    int64_t *isect_ids, uint32_t *keys32, int32_t *flatten_ids, gs_stream_t stream) {
    return emit_presorted_launch(compact ? 1 : 0, 0u, n_elems, N, perm, n_valid, camera_ids, means2d, means2d_stride, radii, depths,
                                 tiles_per_gauss, group_sums, group_prefix, tile_size, tile_width, tile_height, tile_n_bits, isect_ids, keys32,
                                 flatten_ids, stream);
}

// Packed emission: words[i] = (camera << tile_n_bits | tile) << pos_bits | emission position of the splat (its index in perm:
// the depth rank).  Needs key bits + pos_bits <= 32; see gs_sort_isect_packed.
extern "C" int32_t gs_isect_emit_packed(
    uint32_t n_elems, uint32_t N, const int32_t *perm, const uint32_t *n_valid, const int64_t *camera_ids, const float *means2d,
    uint32_t means2d_stride, const int32_t *radii, const float *depths, const int32_t *tiles_per_gauss, const uint32_t *group_sums,
    const int64_t *group_prefix, uint32_t tile_size, uint32_t tile_width, uint32_t tile_height, uint32_t tile_n_bits, uint32_t pos_bits,
    uint32_t *words, gs_stream_t stream) {
    GS_CHECK_ARG(pos_bits + tile_n_bits <= 32, "tile bits + position bits must fit 32 bits");
    return emit_presorted_launch(2, pos_bits, n_elems, N, perm, n_valid, camera_ids, means2d, means2d_stride, radii, depths, tiles_per_gauss,
                                 group_sums, group_prefix, tile_size, tile_width, tile_height, tile_n_bits, nullptr, words, nullptr, stream);
}

extern "C" int32_t gs_isect_offset_encode(
    uint32_t n_isects, const int64_t *isect_ids_sorted, uint32_t C, uint32_t n_tiles,
    uint32_t tile_n_bits, int32_t *offsets, gs_stream_t stream) {
    GS_CHECK_ARG(offsets != nullptr, "null pointer");
    if ((uint64_t)C * n_tiles == 0) return 0;
    if (n_isects == 0) {
        // reference: offsets.fill_(0)  (isect_tiles.cu:385-387)
        hipError_t e = hipMemsetAsync(offsets, 0, (size_t)C * n_tiles * sizeof(int32_t), (hipStream_t)stream);
        if (e != hipSuccess) {
            gs_set_error("gs_isect_offset_encode: memset failed: %s", hipGetErrorString(e));
            return 2;
        }
        return 0;
    }
    GS_CHECK_ARG(isect_ids_sorted != nullptr, "null pointer");
    hipLaunchKernelGGL(isect_offset_encode_kernel, dim3(gs_div_up(n_isects, GS_BLOCK * OFFSET_ITEMS)), dim3(GS_BLOCK), 0,
                       (hipStream_t)stream, n_isects, isect_ids_sorted, C, n_tiles, tile_n_bits, offsets);
    GS_CHECK_LAUNCH();
    return 0;
}

// emit (compact) -> 32-bit pair sort -> offsets, one call: see the header
static size_t finish_pairs_bytes(uint64_t n) { return ((size_t)n * 4 + 255) / 256 * 256; }

extern "C" size_t gs_isect_finish_work_bytes(uint64_t n_isects) {
    return 2 * finish_pairs_bytes(n_isects) + gs_sort_isect_temp_bytes(n_isects);
}

// ---- row binning: layout of its arrays in the work buffer, switch, route query
namespace {
struct RowBinLayout {
    uint32_t n_blocks, max_chunks; // stage-1/3 blocks; upper bound of the chunks: sum ceil(len_r / RB_ITEMS) <= entries / RB_ITEMS + rows
    size_t off_row_cnt, off_row_pairs, off_row_total, off_tables, off_items, off_col_cnt, total;
};
RowBinLayout rowbin_layout(uint64_t n_isects, uint32_t n_kept, uint32_t rows, uint32_t tw) {
    RowBinLayout L;
    L.n_blocks = gs_div_up(n_kept, RB_POS_ITEMS);
    L.max_chunks = (uint32_t)(n_isects / RB_ITEMS) + rows;
    Carve cv;
    cv.take((size_t)n_isects * sizeof(uint2)); // the row entries: at most one per pair (where the word arrays of the other routes live)
    L.off_row_cnt = cv.take((size_t)rows * L.n_blocks * sizeof(uint32_t));
    L.off_row_pairs = cv.take((size_t)rows * L.n_blocks * sizeof(uint32_t));
    L.off_row_total = cv.take((size_t)2 * rows * sizeof(uint32_t)); // entries | pairs of every row
    L.off_tables = cv.take((size_t)3 * (rows + 1) * sizeof(uint32_t)); // row_start | chunk_first | pairs_before
    L.off_items = cv.take((size_t)n_kept * sizeof(uint2));         // stage 1's item per position: rows | columns
    L.off_col_cnt = cv.take((size_t)L.max_chunks * tw * sizeof(uint32_t));
    L.total = cv.total;
    return L;
}
std::atomic<int32_t> g_row_binning{1}, g_last_route{GS_ISECT_ROUTE_NONE};
} // namespace

extern "C" int32_t gs_isect_row_binning(int32_t on) { return on < 0 ? g_row_binning.load() : g_row_binning.exchange(on != 0 ? 1 : 0); }
extern "C" int32_t gs_isect_last_route(void) { return g_last_route.load(); }
extern "C" size_t gs_isect_row_binning_work_bytes(uint64_t n_isects, uint32_t n_kept, uint32_t rows, uint32_t tile_width) {
    return rowbin_layout(n_isects, n_kept, rows, tile_width).total;
}

static int32_t isect_finish_rows(
    uint32_t n_elems, uint32_t N, uint32_t n_isects, const int32_t *perm, const uint32_t *n_valid, const float *means2d, uint32_t s_m2,
    const int32_t *radii, const float *depths, uint32_t tile_size, uint32_t tw, uint32_t th, uint32_t tile_n_bits, uint32_t C,
    int64_t *isect_ids, int32_t *flatten_ids, int32_t *offsets, void *work, const RowBinLayout &L, uint32_t n_kept, const int64_t *sorted_keys,
    hipStream_t st) {
    const uint32_t rows = C * th;
    uint2 *entries = (uint2 *)work;
    uint32_t *row_cnt = (uint32_t *)((char *)work + L.off_row_cnt), *row_pairs = (uint32_t *)((char *)work + L.off_row_pairs);
    uint32_t *row_total = (uint32_t *)((char *)work + L.off_row_total), *col_cnt = (uint32_t *)((char *)work + L.off_col_cnt);
    uint2 *items = (uint2 *)((char *)work + L.off_items);
    uint32_t *tables = (uint32_t *)((char *)work + L.off_tables);
    // the chunk kernels walk the chunks with a stride: the host knows their number only as a bound
    const uint32_t chunk_grid = min(L.max_chunks, 2048u);
    hipLaunchKernelGGL(rb_row_hist_kernel, dim3(L.n_blocks), dim3(GS_BLOCK), 0, st, n_elems, n_kept, N, C, perm, n_valid, means2d, s_m2, radii,
                       (float)tile_size, (int32_t)tw, (int32_t)th, rows, L.n_blocks, row_cnt, row_pairs, items);
    hipLaunchKernelGGL(rb_row_scan_kernel, dim3(rows), dim3(GS_BLOCK), 0, st, rows, L.n_blocks, row_cnt, row_pairs, row_total, tw, offsets);
    hipLaunchKernelGGL(rb_row_scatter_kernel, dim3(L.n_blocks), dim3(GS_BLOCK), 0, st, n_elems, n_kept, n_valid, items, rows, L.n_blocks, row_cnt,
                       row_total, tables, entries, n_isects);
    hipLaunchKernelGGL(rb_col_hist_kernel, dim3(chunk_grid), dim3(GS_BLOCK), 0, st, rows, tw, tables, entries, n_isects, L.max_chunks, col_cnt, offsets);
    hipLaunchKernelGGL(rb_col_scan_kernel, dim3(rows + gs_div_up((uint64_t)rows * tw, RB_WAVES)), dim3(GS_BLOCK), 0, st, rows, tw, tables, L.max_chunks, col_cnt, offsets);
    hipLaunchKernelGGL(rb_expand_kernel, dim3(chunk_grid), dim3(GS_BLOCK), 0, st, n_elems, rows, tw, th, tile_n_bits, tables, entries, n_isects,
                       L.max_chunks, col_cnt, offsets, perm, (const uint64_t *)sorted_keys, depths, n_isects, isect_ids, flatten_ids);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_isect_finish_presorted(
    uint32_t n_elems, uint32_t N, uint64_t n_isects, const int32_t *perm, const uint32_t *n_valid, const int64_t *camera_ids,
    const float *means2d, uint32_t means2d_stride, const int32_t *radii, const float *depths, const int32_t *tiles_per_gauss,
    const uint32_t *group_sums, const int64_t *group_prefix, uint32_t tile_size, uint32_t tile_width, uint32_t tile_height,
    uint32_t tile_n_bits, uint32_t cam_n_bits, uint32_t C, int64_t *isect_ids, int32_t *flatten_ids, int32_t *offsets, void *work,
    size_t work_bytes, uint32_t n_kept_host, const int64_t *sorted_keys, gs_stream_t stream) {
    GS_CHECK_ARG(offsets != nullptr, "null pointer");
    if (n_isects > 0) {
        GS_CHECK_ARG(work != nullptr && (uintptr_t)work % 16 == 0 && work_bytes >= gs_isect_finish_work_bytes(n_isects),
                     "work buffer too small (gs_isect_finish_work_bytes) or misaligned");
        const size_t pb = finish_pairs_bytes(n_isects);
        uint32_t *keys32 = (uint32_t *)work;
        int32_t *vals = (int32_t *)((char *)work + pb);
        void *temp = (char *)work + 2 * pb;
        // PACKED route: the caller knows how many splats the pre-sort kept (n_kept_host, e.g. from the projection's block sums)
        // and (camera, tile) key + emission position fit ONE 32-bit word -- 4 bytes per pair through emission and sort instead
        // of 8, no value array.  The key bits that can be set: the tile bits + the bits of the largest camera index.
        uint32_t pos_bits = 0, cam_bits = 0;
        while (n_kept_host > 0 && ((uint64_t)1 << pos_bits) < (uint64_t)n_kept_host) ++pos_bits;
        while (((uint32_t)1 << cam_bits) < C) ++cam_bits;
        const uint32_t key_bits_eff = tile_n_bits + cam_bits;
        // ROW route: (splat, tile row) entries into row order by one counting pass, rows expanded into columns (see the header).
        // Within its limits, and when its arrays fit the buffer that came in (the query is a function of n_isects alone).
        const uint64_t rows64 = (uint64_t)C * tile_height;
        if (g_row_binning.load() != 0 && n_kept_host > 0 && perm != nullptr && camera_ids == nullptr && key_bits_eff <= 31 &&
            tile_n_bits < 32 && ((uint64_t)tile_width * tile_height >> tile_n_bits) == 0 && N > 0 && tile_size > 0 && means2d != nullptr &&
            radii != nullptr && (sorted_keys != nullptr || depths != nullptr) && isect_ids != nullptr && flatten_ids != nullptr &&
            means2d_stride >= 2 && means2d_stride % 2 == 0 && tile_width >= 1 && tile_width <= GS_ROW_BINNING_MAX_WIDTH && rows64 >= 1 &&
            rows64 <= GS_ROW_BINNING_MAX_ROWS && n_isects < (1ull << 31) &&
            rows64 * gs_div_up(n_kept_host, RB_POS_ITEMS) <= GS_ROW_BINNING_MAX_COUNTERS) {
            const RowBinLayout L = rowbin_layout(n_isects, n_kept_host, (uint32_t)rows64, tile_width);
            if (L.total <= work_bytes) {
                g_last_route.store(GS_ISECT_ROUTE_ROWS);
                return isect_finish_rows(n_elems, N, (uint32_t)n_isects, perm, n_valid, means2d, means2d_stride, radii, depths, tile_size,
                                         tile_width, tile_height, tile_n_bits, C, isect_ids, flatten_ids, offsets, work, L, n_kept_host,
                                         sorted_keys, (hipStream_t)stream);
            }
        }
        if (n_kept_host > 0 && perm != nullptr && camera_ids == nullptr && key_bits_eff >= 1 && key_bits_eff + pos_bits <= 32 &&
            key_bits_eff <= 31) {
            g_last_route.store(GS_ISECT_ROUTE_PACKED);
            int32_t rc = gs_isect_emit_packed(n_elems, N, perm, n_valid, camera_ids, means2d, means2d_stride, radii, depths, tiles_per_gauss,
                                              group_sums, group_prefix, tile_size, tile_width, tile_height, tile_n_bits, pos_bits, keys32, stream);
            if (rc != 0) return rc;
            rc = gs_sort_isect_packed(n_isects, keys32, perm, sorted_keys, depths, (int32_t)key_bits_eff, pos_bits, isect_ids, flatten_ids,
                                      temp, work_bytes - 2 * pb, stream);
            if (rc != 0) return rc;
            return gs_isect_offset_encode((uint32_t)n_isects, isect_ids, C, tile_width * tile_height, tile_n_bits, offsets, stream);
        }
        g_last_route.store(GS_ISECT_ROUTE_PAIRS);
        int32_t rc = gs_isect_emit_presorted(n_elems, N, perm, n_valid, camera_ids, means2d, means2d_stride, radii, depths, tiles_per_gauss,
                                             group_sums, group_prefix, tile_size, tile_width, tile_height, tile_n_bits, 1, nullptr,
                                             keys32, vals, stream);
        if (rc != 0) return rc;
        // (only the bits a key can have set take part: 8 cameras are 3 bits, not the 4 of the id layout -- 16 key bits = two passes
        // instead of three; with all 32 bits in use the last pass also orders the ids as the signed values they are: left alone)
        const uint32_t sort_bits = (tile_n_bits + cam_n_bits < 32u && key_bits_eff >= 1u) ? key_bits_eff : tile_n_bits + cam_n_bits;
        rc = gs_sort_isect_pairs(n_isects, keys32, vals, depths, (int32_t)sort_bits, isect_ids, flatten_ids, temp,
                                 work_bytes - 2 * pb, stream);
        if (rc != 0) return rc;
    }
    return gs_isect_offset_encode((uint32_t)n_isects, isect_ids, C, tile_width * tile_height, tile_n_bits, offsets, stream);
}
