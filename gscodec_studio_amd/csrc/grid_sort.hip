// grid_sort.hip -- the rounds of the grid sort: the order of the splats on the S x S image grid of the PNG codecs that makes
// every attribute image smooth (gfx950).
//
// The reference takes this ordering from the `plas` package (gsplat/compression/sort.py); here the algorithm is the library's
// own, defined by the numpy code gscodec_studio_amd/compression/grid_sort_reference.py, and every kernel below is integer
// arithmetic whose result equals it element for element.  One round at radius r:
//
//   gs_gridsort_blur    target = box blur (width w = 2 r + 1, reflect borders) of the 12-bit features gathered through `order`:
//                       rows, then columns, each pass an exact window sum s and (2 s + w) / (2 w)
//   gs_gridsort_keys    key(p) = block(p) << 32 | hash(seed, k, p) over randomly shifted blocks of side b; value p
//   gs_sort_pairs_u64_i32 (radix_sort.hip) over the populated bits: runs of four positions of one block, in random order
//   gs_gridsort_assign  one lane per run: the best of the 24 assignments of its four items to its four targets
//
// The blur is a sliding window: a lane owns one (line, channel, segment of at most 128 outputs), sums its first window (w
// independent loads) and then adds one element and drops one per output, so a pass costs w + 2 * segment loads per lane and not
// w per output.  Lanes run over the channel first: in the column pass a wave reads and writes consecutive addresses, in the row
// pass the C lanes of a position share one gathered row of q.  Shorter segments at small radii keep the number of lanes up
// where the first window is cheap.
#include "gs_common.h"

namespace {

constexpr uint32_t GRIDSORT_MAX_C = 64;
constexpr uint32_t GRIDSORT_MAX_S = 46340; // S * S < 2^31: positions and splat indices are int32

// The text of hash32 in grid_sort_reference.py (murmur3's finaliser, twice), uint32 arithmetic.
__host__ __device__ inline uint32_t gridsort_hash(uint32_t seed, uint32_t k, uint32_t p) {
    const uint32_t GOLD = 0x9E3779B9u, MIX1 = 0x85EBCA6Bu, MIX2 = 0xC2B2AE35u, ONE = 1u;
    uint32_t x;
    x = seed + (k + ONE) * GOLD;
    x ^= x >> 16;
    x *= MIX1;
    x ^= x >> 13;
    x *= MIX2;
    x ^= x >> 16;
    x = x ^ (p * MIX1);
    x ^= x >> 16;
    x *= MIX1;
    x ^= x >> 13;
    x *= MIX2;
    x ^= x >> 16;
    return x;
}

// numpy's pad(mode="reflect") for -(S - 1) <= i <= 2 (S - 1): the border element is not repeated
__host__ __device__ inline uint32_t gridsort_reflect(int32_t i, int32_t S) {
    i = i < 0 ? -i : i;
    return (uint32_t)(i >= S ? 2 * (S - 1) - i : i);
}

// ROW: line = y, the window runs along x and the input is q gathered through order; otherwise line = x, the window runs
// along y over the row pass's output.  Sums: w * 4095 <= (2 * 46339 + 1) * 4095 < 2^29, so 2 s + w fits 32 bits.
template <bool ROW>
__global__ void __launch_bounds__(GS_BLOCK) gridsort_blur_kernel(uint32_t S, uint32_t C, uint32_t r, uint32_t seg_len, uint32_t n_seg,
                                                                 const uint16_t *__restrict__ in, const int32_t *__restrict__ order,
                                                                 uint16_t *__restrict__ out) {
    const uint64_t per_seg = (uint64_t)S * C;
    const uint64_t tid = (uint64_t)blockIdx.x * GS_BLOCK + threadIdx.x;
    if (tid >= per_seg * n_seg) return;
    const uint32_t seg = (uint32_t)(tid / per_seg);
    const uint32_t j = (uint32_t)(tid - (uint64_t)seg * per_seg);
    const uint32_t line = j / C, c = j - line * C;
    const uint32_t N = S * S;
    auto pos = [&](uint32_t i) { return ROW ? line * S + i : i * S + line; };
    auto at = [&](int32_t i) -> uint32_t {
        const uint32_t p = pos(gridsort_reflect(i, (int32_t)S));
        if (ROW) {
            const uint32_t o = (uint32_t)order[p];
            return in[(uint64_t)(o < N ? o : N - 1u) * C + c]; // an entry that is no splat index must not leave q
        }
        return in[(uint64_t)p * C + c];
    };
    const int32_t x0 = (int32_t)(seg * seg_len);
    const int32_t x1 = (int32_t)(x0 + seg_len < S ? x0 + seg_len : S);
    const int32_t ri = (int32_t)r;
    const uint32_t w = 2u * r + 1u;
    uint32_t s = 0u;
#pragma unroll 8
    for (int32_t i = x0 - ri; i <= x0 + ri; ++i) s += at(i);
    for (int32_t x = x0; x < x1; ++x) {
        out[(uint64_t)pos((uint32_t)x) * C + c] = (uint16_t)((2u * s + w) / (2u * w));
        if (x + 1 < x1) s += at(x + 1 + ri) - at(x - ri);
    }
}

__global__ void __launch_bounds__(GS_BLOCK) gridsort_keys_kernel(uint32_t S, uint32_t b, uint32_t seed, uint32_t k,
                                                                 int64_t *__restrict__ keys, int32_t *__restrict__ vals) {
    const uint32_t N = S * S;
    const uint32_t p = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (p >= N) return;
    uint32_t block = 0u;
    if (b != 0u) {
        const uint32_t ox = gridsort_hash(seed, k, N) % b, oy = gridsort_hash(seed, k, N + 1u) % b;
        const uint32_t y = p / S, x = p - y * S;
        block = ((y + oy) / b) * (S / b + 2u) + (x + ox) / b;
    }
    keys[p] = (int64_t)(((uint64_t)block << 32) | gridsort_hash(seed, k, p));
    vals[p] = (int32_t)p;
}

// itertools.permutations(range(4)): lexicographic, the identity first
__device__ constexpr uint8_t GRIDSORT_PERMS[24][4] = {
    {0, 1, 2, 3}, {0, 1, 3, 2}, {0, 2, 1, 3}, {0, 2, 3, 1}, {0, 3, 1, 2}, {0, 3, 2, 1}, {1, 0, 2, 3}, {1, 0, 3, 2},
    {1, 2, 0, 3}, {1, 2, 3, 0}, {1, 3, 0, 2}, {1, 3, 2, 0}, {2, 0, 1, 3}, {2, 0, 3, 1}, {2, 1, 0, 3}, {2, 1, 3, 0},
    {2, 3, 0, 1}, {2, 3, 1, 0}, {3, 0, 1, 2}, {3, 0, 2, 1}, {3, 1, 0, 2}, {3, 1, 2, 0}, {3, 2, 0, 1}, {3, 2, 1, 0}};

// PAIR: C is even, so every row of q and of the target starts on a 32-bit word and two channels travel per load
template <bool PAIR>
__global__ void __launch_bounds__(GS_BLOCK) gridsort_assign_kernel(uint32_t N, uint32_t C, const uint16_t *__restrict__ q,
                                                                   const uint16_t *__restrict__ target,
                                                                   const int64_t *__restrict__ sorted_keys,
                                                                   const int32_t *__restrict__ sorted_pos,
                                                                   const int32_t *__restrict__ order_in, int32_t *__restrict__ order_out) {
    const uint32_t g = blockIdx.x * GS_BLOCK + threadIdx.x;
    if ((uint64_t)g * 4u >= N) return;
    const uint32_t base = g * 4u;
    const uint32_t cnt = N - base < 4u ? N - base : 4u;
    uint32_t P[4];
    int32_t O[4];
    bool regroup = cnt == 4u; // the trailing N % 4 positions keep their entries
    const uint32_t blk0 = (uint32_t)((uint64_t)sorted_keys[base] >> 32);
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        if (i < cnt) {
            const uint32_t p = (uint32_t)sorted_pos[base + i];
            P[i] = p < N ? p : N - 1u; // whatever the sort left there, no access leaves the arrays
            O[i] = order_in[P[i]];
            regroup = regroup && (uint32_t)((uint64_t)sorted_keys[base + i] >> 32) == blk0; // a run that straddles two blocks
        } else {
            P[i] = 0u;
            O[i] = 0;
        }
    }
    if (!regroup) {
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i)
            if (i < cnt) order_out[P[i]] = O[i];
        return;
    }
    // d[i][j] = sum over the channels of (item i - target j)^2 <= 64 * 4095^2 = 1 073 217 600 < 2^31: exact in 32 bits.  The
    // sum of four of them can reach 4 292 870 400, 2 096 896 short of 2^32: it is taken in 64 bits rather than lean on that.
    uint32_t d[4][4] = {};
    uint64_t ra[4], rt[4];
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        const uint32_t o = (uint32_t)O[i];
        ra[i] = (uint64_t)(o < N ? o : N - 1u) * C;
        rt[i] = (uint64_t)P[i] * C;
    }
    if (PAIR) {
        const uint32_t *q2 = (const uint32_t *)q, *t2 = (const uint32_t *)target;
        for (uint32_t c = 0; c < C / 2u; ++c) {
            uint32_t a[4], t[4];
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) {
                a[i] = q2[ra[i] / 2u + c];
                t[i] = t2[rt[i] / 2u + c];
            }
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i)
#pragma unroll
                for (uint32_t jj = 0; jj < 4u; ++jj) {
                    const int32_t lo = (int32_t)(a[i] & 0xFFFFu) - (int32_t)(t[jj] & 0xFFFFu);
                    const int32_t hi = (int32_t)(a[i] >> 16) - (int32_t)(t[jj] >> 16);
                    d[i][jj] += (uint32_t)(lo * lo) + (uint32_t)(hi * hi);
                }
        }
    } else {
        for (uint32_t c = 0; c < C; ++c) {
            int32_t a[4], t[4];
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) {
                a[i] = (int32_t)q[ra[i] + c];
                t[i] = (int32_t)target[rt[i] + c];
            }
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i)
#pragma unroll
                for (uint32_t jj = 0; jj < 4u; ++jj) d[i][jj] += (uint32_t)((a[i] - t[jj]) * (a[i] - t[jj]));
        }
    }
    uint64_t best = ~0ull;
    uint32_t D[4] = {P[0], P[1], P[2], P[3]}; // where item i goes
#pragma unroll
    for (uint32_t m = 0; m < 24u; ++m) {
        const uint8_t *pm = GRIDSORT_PERMS[m];
        const uint64_t cost = (uint64_t)d[0][pm[0]] + d[1][pm[1]] + d[2][pm[2]] + d[3][pm[3]];
        if (cost < best) { // strict: the first minimum, so a tie keeps the earlier permutation (the identity among them)
            best = cost;
            D[0] = P[pm[0]];
            D[1] = P[pm[1]];
            D[2] = P[pm[2]];
            D[3] = P[pm[3]];
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) order_out[D[i]] = O[i];
}

bool gridsort_shape_ok(uint32_t S, uint32_t C) { return S >= 1 && S <= GRIDSORT_MAX_S && C >= 1 && C <= GRIDSORT_MAX_C; }

} // namespace

extern "C" int32_t gs_gridsort_blur(uint32_t S, uint32_t C, uint32_t r, const uint16_t *q, const int32_t *order, uint16_t *tmp,
                                    uint16_t *target, gs_stream_t stream) {
    GS_CHECK_ARG(gridsort_shape_ok(S, C), "need 1 <= S <= 46340 and 1 <= C <= 64");
    GS_CHECK_ARG(r >= 1 && r < S, "need 1 <= r < S (reflect borders)");
    GS_CHECK_ARG(q && order && tmp && target, "null pointer");
    GS_CHECK_ARG(tmp != target && (const uint16_t *)tmp != q && (const uint16_t *)target != q, "q, tmp and target must be three buffers");
    const uint32_t w = 2u * r + 1u;
    const uint32_t seg_len = w < 16u ? 16u : (w > 128u ? 128u : w); // a lane's first window costs w loads: no more than 3 x the sliding part
    const uint32_t n_seg = gs_div_up(S, seg_len);
    const uint64_t threads = (uint64_t)S * C * n_seg;
    GS_CHECK_ARG((threads + GS_BLOCK - 1) / GS_BLOCK < (1ull << 31), "grid too large");
    const dim3 grid(gs_div_up(threads, GS_BLOCK));
    hipLaunchKernelGGL(gridsort_blur_kernel<true>, grid, dim3(GS_BLOCK), 0, (hipStream_t)stream, S, C, r, seg_len, n_seg, q, order, tmp);
    hipLaunchKernelGGL(gridsort_blur_kernel<false>, grid, dim3(GS_BLOCK), 0, (hipStream_t)stream, S, C, r, seg_len, n_seg,
                       (const uint16_t *)tmp, (const int32_t *)nullptr, target);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_gridsort_keys(uint32_t S, uint32_t b, uint32_t seed, uint32_t k, int64_t *keys, int32_t *vals, gs_stream_t stream) {
    GS_CHECK_ARG(S >= 1 && S <= GRIDSORT_MAX_S, "need 1 <= S <= 46340");
    GS_CHECK_ARG(keys && vals, "null pointer");
    hipLaunchKernelGGL(gridsort_keys_kernel, dim3(gs_div_up((uint64_t)S * S, GS_BLOCK)), dim3(GS_BLOCK), 0, (hipStream_t)stream, S, b, seed, k,
                       keys, vals);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_gridsort_assign(uint32_t S, uint32_t C, const uint16_t *q, const uint16_t *target, const int64_t *sorted_keys,
                                      const int32_t *sorted_pos, const int32_t *order_in, int32_t *order_out, gs_stream_t stream) {
    GS_CHECK_ARG(gridsort_shape_ok(S, C), "need 1 <= S <= 46340 and 1 <= C <= 64");
    GS_CHECK_ARG(q && target && sorted_keys && sorted_pos && order_in && order_out, "null pointer");
    GS_CHECK_ARG(order_in != order_out, "order_out must not alias order_in");
    GS_CHECK_ARG(((uintptr_t)q | (uintptr_t)target) % 4u == 0, "q and target must be 4-byte aligned");
    const uint32_t N = S * S;
    const dim3 grid(gs_div_up(gs_div_up(N, 4), GS_BLOCK));
    if (C % 2u == 0u)
        hipLaunchKernelGGL(gridsort_assign_kernel<true>, grid, dim3(GS_BLOCK), 0, (hipStream_t)stream, N, C, q, target, sorted_keys,
                           sorted_pos, order_in, order_out);
    else
        hipLaunchKernelGGL(gridsort_assign_kernel<false>, grid, dim3(GS_BLOCK), 0, (hipStream_t)stream, N, C, q, target, sorted_keys,
                           sorted_pos, order_in, order_out);
    GS_CHECK_LAUNCH();
    return 0;
}
