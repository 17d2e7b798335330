// scan_dev.h -- the building blocks the tile-binning chain shares (isect.hip, radix_sort.hip): wave and workgroup prefix sums,
// segmented side sums, the pair id read off the depth order, and the host-side carve of a work buffer.
// (rasterize.hip and exchange.hip keep scan loops of their own: other flags, measured separately.)
#pragma once
#include "gs_common.h"

// Offsets of consecutive arrays in one work buffer, each starting on a 256-byte boundary; `total` is the buffer's size.
struct Carve {
    size_t total = 0;
    size_t take(size_t bytes) {
        const size_t at = total;
        total += (bytes + 255) & ~(size_t)255;
        return at;
    }
};

#ifdef __HIPCC__
// inclusive prefix sum over the 64 lanes of a wave: int32_t, uint32_t, int64_t
// (the lane from lane_id(), which the shuffles compute anyway: threadIdx.x % 64 cost up to 21 instructions more per kernel)
template <typename T>
GS_DEV T wave_inclusive_scan(T v) {
    const uint32_t lane = lane_id();
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T o = __shfl_up(v, off, 64);
        if (lane >= (uint32_t)off) v += o;
    }
    return v;
}

template <typename T>
struct BlockScan {
    T inc, exc, total; // inclusive and exclusive prefix of the thread's value, sum over the workgroup
};

// Prefix sum of one value per thread over the first WAVES waves of the workgroup (4 or 16); a workgroup with more waves passes
// 0 in the others, which get the total as their prefix.  Every thread of the workgroup calls it.
// Contract: s_w (WAVES values) is free on entry -- a barrier lies between its last use and the call -- and free again on
// return.  Two workgroup barriers: one after the wave totals are written, one after they are read.
template <uint32_t WAVES, typename T>
GS_DEV BlockScan<T> block_scan(T v, T *s_w) {
    const uint32_t lane = threadIdx.x % GS_WAVE, wave = threadIdx.x / GS_WAVE;
    BlockScan<T> r;
    r.inc = wave_inclusive_scan(v);
    if (lane == GS_WAVE - 1 && wave < WAVES) s_w[wave] = r.inc;
    __syncthreads();
    T base = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < WAVES; ++w) {
        const T t = s_w[w];
        if (w < wave) base += t;
        total += t;
    }
    __syncthreads();
    r.inc += base;
    r.exc = r.inc - v;
    r.total = total;
    return r;
}

// Segmented wave sums of `inc` over runs of equal `grp` among consecutive lanes, one atomic per run: consecutive lanes hold
// consecutive output positions, i.e. mostly the same group -- one atomic per (wave, run) instead of one per key on a shared
// counter.  Whole waves call it; lanes that are not `on` add nothing.
GS_DEV void segmented_side_add(uint32_t *side_sums, bool on, uint32_t grp, uint32_t inc) {
    const uint32_t lane = threadIdx.x % GS_WAVE;
    if (!on) { grp = 0xffffffffu; inc = 0u; }
    inc = wave_inclusive_scan(inc);
    const uint32_t prevg = __shfl_up(grp, 1, 64);
    const bool head = lane == 0u || grp != prevg;
    const unsigned long long hm = __ballot(head);
    const unsigned long long above = lane == 63u ? 0ull : (hm >> (lane + 1u));
    const uint32_t last = above ? lane + (uint32_t)__builtin_ctzll(above) : 63u; // last lane of my run
    const uint32_t upto = __shfl(inc, (int)last, 64);
    const uint32_t before = __shfl_up(inc, 1, 64);
    if (head && on) atomicAdd(&side_sums[grp], upto - (lane == 0u ? 0u : before));
}

// Flatten id and depth bits of the splat at position `pos` of the depth order, for the 64-bit pair id
//   key << 32 | (int64_t)depth_bits   (the reference's (int64_t)*(int32_t*)&depth, isect_tiles.cu:91).
// sorted_keys (or NULL): the pre-sort's (depth bits << 32 | element) keys by position -- both in ONE 8-byte gather (depths of
// visible splats are positive: their bits ARE the key's high half) instead of the dependent pair perm[pos] -> depths[id].
GS_DEV void pair_id_of(uint32_t pos, const uint64_t *__restrict__ sorted_keys, const int32_t *__restrict__ perm,
                       const float *__restrict__ depths, int32_t *flatten_id, int32_t *depth_bits) {
    if (sorted_keys != nullptr) { // (uniform)
        const uint64_t sk = sorted_keys[pos];
        *flatten_id = (int32_t)(uint32_t)sk;
        *depth_bits = (int32_t)(uint32_t)(sk >> 32);
    } else {
        *flatten_id = perm[pos];
        *depth_bits = __float_as_int(depths[*flatten_id]);
    }
}
#endif
