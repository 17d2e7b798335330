// rasterize.hip -- per-tile front-to-back alpha compositing, forward and backward, for gfx950.
//
// Replaces gsplat/cuda/csrc/rasterize_to_pixels_fwd.cu:16-185 and rasterize_to_pixels_bwd.cu:17-277.  Same per-pixel arithmetic
// and decisions (alpha = min(0.999, o * exp(-sigma)); skip sigma < 0 or alpha < 1/255; exclusive stop when T (1 - alpha) <= 1e-4;
// last_ids; alpha-clamp gradient gate -- splat_sample and the constants beside it in rasterize_dev.h, the one definition every
// kernel here and in rasterize_wide.hip uses), different mapping.  Common to every kernel:
//
//   * A tile of up to 16x16 pixels is four 8x8 QUADRANTS; one wave64 composites one quadrant, lane (lx, ly) = one pixel.
//   * LDS-STAGED, CULLED SPLAT LISTS: a lane gathers one splat of the tile's sorted list (flatten_ids -> means2d / conics /
//     opacities / colours) and converts it to what the inner loop wants: the conic pre-scaled by -log2(e)/2 so that
//         alpha = exp2(dx (a' dx + b' dy) + c' dy^2 + log2 o)      (5 FMA + v_exp_f32).
//     While it holds the splat it tests, exactly, whether { alpha >= 1/255 } reaches the live pixel rectangle of a quadrant
//     (cull_prepare / rect_touch); only the survivors are written to LDS, in list order.  A culled splat has alpha < 1/255 at
//     every pixel of the rectangle, which the reference skips too.  The next batch's gathers are issued before the current
//     batch is walked (software prefetch).
//   * The longest lists bound the critical path (their waves run alone at the end of a kernel): those waves run at raised
//     priority (s_setprio).
//
// Three kernel families:
//
//   1. TILE FORWARD, raster_tile_fwd_kernel<CDIM, CKPT>: one 256-thread workgroup per tile, wave q composites quadrant q, the
//      colours travel in the LDS record.  1..4 channels in one launch (CDIM = channels), 5..16 in one launch of the wide
//      instances (8, 9, 12, 16), 17..32 as two launches over halves.  The four waves stage cooperatively, or -- the longest
//      lists -- each for itself (SOLO).  CKPT: per-pixel checkpoints every `seg` list entries and the cost of every
//      (tile, segment) item, for the segmented backward.  Its stages (pixel of a lane, masked tile, priority, record write,
//      checkpoint cursor, list index of a record, epilogue) are defined once, in rasterize_dev.h.
//   2. GENERIC WAVE FORWARD / BACKWARD, raster_wave_fwd_kernel<CDIM> / raster_wave_bwd_kernel<CDIM, CMODE, ABS>: one
//      independent wave per (tile, quadrant), no workgroup barriers, colours of 5 and more channels read from global memory at
//      wave-uniform addresses.  The forward without a plan (a C-ABI caller without scratch) and beyond 32 channels, in exact
//      chunks of 32; the backward whenever there are no checkpoints, and beyond 32 channels in ONE pass (v_out re-read per
//      splat) so that v_alpha -- and therefore absgrad -- sees every channel, as the reference's single kernel does.
//   3. SEGMENTED BACKWARDS, raster_seg_bwd_kernel<CDIM, ABS, DET> here (1..4 channels) and raster_seg_bwd_wide_kernel in
//      rasterize_wide.hip (5..32): one wave per (tile, segment) item restarts from the forward's checkpoint; the items run
//      longest first (seg_items_build_kernel).  Their shared stages: rasterize_seg_dev.h.
//
// Backward, per (pixel, splat) with the running transmittance T and
//         D = sum_k colour_k v_out_k,   B = sum_{splats behind} fac D   (a scalar),
//     v_alpha = D T + (T_final (v_alpha_out - bg . v_out) - B) / (1 - alpha) -- the reference's per-channel "buffer" vector
//     (rasterize_to_pixels_bwd.cu:203-241) collapses to the scalar B, so the per-pixel state does not grow with the channel
//     count.  Every lane accumulates the moments
//       S0 = sum v_sigma, Sx = sum v_sigma dx, Sy, Sxx, Sxy, Syy   and   C_k = sum fac v_out_k;
//     one DPP reduction per value per (tile, splat), then
//       v_xy = (a Sx + b Sy, b Sx + c Sy), v_conic = (Sxx/2, Sxy, Syy/2), v_opacity = -S0 / o,
//     v_colour = C: algebraically the reference's formulas (bwd.cu:221-236) with the per-pixel conic products hoisted out of
//     the pixel loop.
#include "gs_common.h"
#include "rasterize_common.h"
#include "dpp_reduce.h"

#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "rasterize_seg_dev.h"

namespace {

// ---------------------------------------------------------------------------
// generic forward (no plan, or more than 32 channels in chunks of 32): one wave per quadrant (vitem & 3) of a tile, the
// colours of channels [ch_off, ch_off + cnt), cnt <= CDIM, read from global memory at wave-uniform addresses
// record: R0 = (mx, my, a', b')  R1 = (c', log2 o, 0, 0)  R2 = (0, 0, idx, g)
// ---------------------------------------------------------------------------
template <int CDIM>
__global__ void __launch_bounds__(GS_WAVE) raster_wave_fwd_kernel(RasterArgs a, uint32_t cnt, uint32_t ch_off) {
    constexpr int REC = 3;
    __shared__ float4 s_rec[(GS_WAVE + 1) * REC];
    const uint32_t lane = threadIdx.x;
    const uint32_t lx = lane & 7u, ly = lane >> 3;
    const uint32_t vitem = xcd_remap(blockIdx.x, gridDim.x, a.xcd_group);
    const TileGeom tg = tile_geom(a, vitem >> 2);
    const uint32_t q = vitem & 3u;
    const float *bg = a.backgrounds ? a.backgrounds + (size_t)tg.cam * a.channels + ch_off : nullptr;

    const LanePixel p = lane_pixel(a, tg, q, lx, ly);
    const float px = p.px, py = p.py;

    if (a.masks != nullptr && !a.masks[tg.lin]) {
        if (p.inside) store_masked_pixel<0>(a.render_colors, p.pix, a.channels, ch_off, cnt, bg);
        return;
    }

    float T = 1.f, Tkeep = 1.f, out[CDIM];
    int32_t cur = 0;
    bool done = !p.inside;
#pragma unroll
    for (int k = 0; k < CDIM; ++k) out[k] = 0.f;

    const Rect rect = wave_rect(a, tg, q);
    const int32_t n = rect.empty ? 0 : tg.range_end - tg.range_start;
    const int32_t base0 = tg.range_start & ~(GS_WAVE - 1);
    const int32_t num_batches = n > 0 ? (tg.range_end - base0 + GS_WAVE - 1) / GS_WAVE : 0;
    raise_priority_for(n);
    auto in_range = [&](int32_t idx) { return idx >= tg.range_start && idx < tg.range_end && n > 0; };

    SplatRaw nxt = gather_splat(a, base0 + (int32_t)lane, in_range(base0 + (int32_t)lane));
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));

    for (int32_t b = 0; b < num_batches; ++b) {
        const int32_t batch_start = base0 + b * GS_WAVE;
        // ---- cull + compact the prefetched splats into LDS
        SplatRaw s = nxt;
        CullSplat cs;
        const bool have = in_range(batch_start + (int32_t)lane);
        const bool live = have && cull_prepare(s, cs) && rect_touch(s, cs, rect.x0, rect.x1, rect.y0, rect.y1);
        const unsigned long long lm = __ballot(live);
        const int count = __popcll(lm);
        if (live) {
            const int slot = __popcll(lm & lt_mask);
            write_record<0>(&s_rec[slot * REC], s, nullptr); // the colours stay in global memory
            s_rec[slot * REC + 2] = make_float4(0.f, 0.f, __int_as_float(batch_start + (int32_t)lane), __int_as_float(s.g));
        }
        // ---- prefetch the next batch
        if (b + 1 < num_batches) {
            const int32_t ni = batch_start + GS_WAVE + (int32_t)lane;
            nxt = gather_splat(a, ni, in_range(ni));
        }
        __builtin_amdgcn_wave_barrier();

        // ---- walk the compacted records, two per iteration.  The only loop-carried dependency
        // is ONE fma per record (T <- T - T a): a finished pixel keeps multiplying (its
        // contributions are masked by `done`, its final transmittance is parked in Tkeep), so the
        // alpha evaluation of the next records overlaps the composite of the current one.
        auto composite = [&](const float4 &c0, const float4 &c1, const float4 &c2) {
            float col[CDIM];
            const float *cp = a.colors + (size_t)__float_as_int(c2.w) * a.s_color + ch_off;
#pragma unroll
            for (int k = 0; k < CDIM; ++k) col[k] = (uint32_t)k < cnt ? cp[k] : 0.f;
            const int32_t idx = __float_as_int(c2.z);
            const float dx = c0.x - px, dy = c0.y - py;
            SplatSample sm;
            const bool ok = splat_sample(dx, dy, c0.z, c0.w, c1.x, c1.y, sm);
            const float a_eff = ok ? sm.alpha : 0.f;
            const float Tj = T;
            const float next_T = Tj - Tj * a_eff;     // the loop-carried chain
            const bool stop = ok && (next_T <= GS_T_MIN); // exclusive stop
            const bool use = !done && !stop;           // this record is composited
            Tkeep = done ? Tkeep : Tj;                 // transmittance before the stopping splat
            const float vis = use ? a_eff * Tj : 0.f;
#pragma unroll
            for (int k = 0; k < CDIM; ++k) out[k] += col[k] * vis;
            cur = (use && ok) ? idx : cur;
            done = done || stop;
            T = next_T;
        };
        {
            int j = 0;
            for (; j + 1 < count; j += 2) {
                const float4 a0 = s_rec[j * REC + 0], a1 = s_rec[j * REC + 1], a2 = s_rec[j * REC + 2];
                const float4 b0 = s_rec[j * REC + 3], b1 = s_rec[j * REC + 4], b2 = s_rec[j * REC + 5];
                composite(a0, a1, a2);
                composite(b0, b1, b2);
            }
            if (j < count) {
                const float4 a0 = s_rec[j * REC + 0], a1 = s_rec[j * REC + 1], a2 = s_rec[j * REC + 2];
                composite(a0, a1, a2);
            }
        }
        // ---- early exit when every pixel of the wave is finished
        if (__all(done)) break;
        __builtin_amdgcn_wave_barrier();
    }

    if (p.inside) store_pixel<CDIM>(a, p.pix, a.channels, ch_off, cnt, true, done ? Tkeep : T, out, cur, bg);
}

// ---------------------------------------------------------------------------
// Forward for 1..4 channels (the hot case, default): ONE 256-THREAD WORKGROUP PER TILE, wave q
// composites quadrant q, and the four waves STAGE COOPERATIVELY: per batch of 256 list entries
// every thread gathers ONE entry, tests it exactly against all four quadrant rectangles
// (rect_touch) and writes its record once; four ballots per wave give one 64-bit mask per
// (64-entry sub-batch, quadrant) and, through mbcnt, a compacted list of record offsets per
// (sub-batch, quadrant).  After one barrier, wave q walks "its" four lists and reads the records
// as LDS broadcasts.
// Why (measured with per-wave timestamps): with one independent wave per
// quadrant the kernel's duration was the life of the heaviest waves (list 5-6k entries, 311 us of
// a 320 us kernel), and ~60% of that was the exposed latency of the two dependent gathers
// (flatten_ids -> splat) once per 64 entries, because culling leaves only ~15 records to
// evaluate per batch.  Here a heavy tile takes 4x fewer, 4x larger batches, the gathers are
// prefetched two levels deep (ids two batches ahead, splat data one batch ahead) and are hidden
// behind ~60 record evaluations, and every entry is gathered once per tile instead of four times.
// LDS is double-buffered so that one LDS-only barrier per batch suffices.
// Sub-batches are aligned to multiples of 64 of the GLOBAL list index, so a checkpoint boundary
// (multiple of seg) always coincides with a sub-batch start.
// ---------------------------------------------------------------------------
// WIDE (5 <= CDIM <= 16, round 5): the same kernel for feature rendering -- the record grows by the colours
// (REC = 2 + ceil((CDIM - 2) / 4) float4: 64 B at 9 channels, 96 B at 16), the walk takes two records per iteration instead of
// four (the colour FMAs are independent work already, and four records of 6 float4 would not fit the registers), the launch
// covers channels [ch_off, ch_off + cnt) of a.channels (cnt <= CDIM; 17..32 channels = two launches over halves: render_alphas /
// last_ids / costs / the T plane of the checkpoints are written by the first), checkpoints are [k][1 + a.channels][256].
#ifndef GS_WIDE_FWD_WAVES
#define GS_WIDE_FWD_WAVES 4 // waves per SIMD the 12- / 16-channel instances are held to (A/B at 16 channels: 1 = 419 us, 4 = 406, 5 = 480 with spills)
#endif
template <int CDIM, bool CKPT>
__global__ void __launch_bounds__(256, CDIM > 9 ? GS_WIDE_FWD_WAVES : 1) raster_tile_fwd_kernel(RasterArgs a, float *__restrict__ ckpt, int32_t seg, int32_t solo_min,
                                                              uint32_t *__restrict__ cost_head, uint32_t *__restrict__ cost_body,
                                                              uint32_t *__restrict__ body_tile, int32_t *__restrict__ tile_last,
                                                              uint32_t *__restrict__ class_count, ZeroFill zf, uint32_t ch_off, uint32_t cnt) {
    constexpr bool WIDE = CDIM > 4;
    constexpr int NCW = WIDE ? (CDIM - 2 + 3) / 4 : 0; // float4s of colours 2.. behind R0, R1
    constexpr int REC = WIDE ? 2 + NCW : 3;
    constexpr int BATCH = 256;
    // record buffers: 2 (staging of batch b + 1 overlaps the compositing of batch b across the four waves: one barrier per batch);
    // the 12- and 16-channel instances take ONE (half the LDS -- 27 instead of 54 KB at 16 channels, i.e. no longer 3 workgroups
    // per CU -- for a second barrier per batch: 537 -> 415 us at 16 channels; at 9 channels a wash, 275 vs 281)
    constexpr int NBUF = (WIDE && CDIM > 9) ? 1 : 2;
    static_assert((NBUF * BATCH * REC + REC) * 16 < 65536, "record offsets are 16-bit");
    // records of both buffers in ONE array + a null record (alpha = 0) that pads every list to a multiple of four
    __shared__ float4 s_rec[NBUF * BATCH * REC + REC];
    constexpr uint32_t NULL_REC_OFF = (uint32_t)NBUF * BATCH * REC * 16u; // byte offset of the null record
    // per (buffer, sub-batch, quadrant): byte offsets (into s_rec) of the records that touch the quadrant, in list order
    typedef uint16_t list_t; // 16-bit entries keep the workgroup under 32 KB of LDS (5 per CU); 32-bit ones measured 0.252 vs 0.244 ms
    __shared__ __attribute__((aligned(16))) list_t s_list[NBUF][4][4][72];
    __shared__ unsigned long long s_mask[NBUF][4][4]; // [buffer][sub-batch (= staging wave)][quadrant]
    __shared__ uint32_t s_done[NBUF][4];              // [buffer][quadrant]
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6); // staging sub-batch AND composited quadrant
    const uint32_t lx = lane & 7u, ly = lane >> 3;
    if (tid < REC) s_rec[NBUF * BATCH * REC + tid] = make_float4(0.f, tid == 1 ? -__builtin_inff() : 0.f, 0.f, 0.f); // log2(opacity) = -inf
    // the class counters of the backward's work list (seg_items_build_kernel runs after this kernel, in the same call)
    // (a chunked forward -- 17..32 channels as two launches -- writes the counters and the costs in its FIRST launch only: culling does
    // not depend on the channel, and the second launch would only repeat the same stores)
    const bool cost_owner = !WIDE || ch_off == 0u;
    if (CKPT && cost_owner && blockIdx.x == 0 && tid < (uint32_t)COST_CLASSES) class_count[tid] = 0u;
    const TileGeom tg = tile_geom(a, a.tile_order != nullptr ? a.tile_order[blockIdx.x] : xcd_remap(blockIdx.x, gridDim.x, a.xcd_group));
    // the channel window [ch0, ch0 + nch) of this launch in the CH channels of the output image / checkpoint planes
    const uint32_t CH = WIDE ? a.channels : (uint32_t)CDIM, ch0 = WIDE ? ch_off : 0u, nch = WIDE ? cnt : (uint32_t)CDIM;
    const float *bg = a.backgrounds ? a.backgrounds + (size_t)tg.cam * a.channels + ch0 : nullptr;

    const LanePixel p = lane_pixel(a, tg, w, lx, ly);
    const bool inside = p.inside;
    const float px = p.px, py = p.py;

    // Side job: this workgroup's slice of the buffer the matching backward will accumulate into (zf, see gs_rasterize_fwd).
    // Issued as the workgroup's LAST instructions: nothing waits for the stores, and the memory pipes are mostly idle
    // while the chip composites -- the separate 64 MB fill kernel (+ its launch gap) of the backward disappears.
    // (Issued right after the first gathers instead: 201 -> 225 us with a 300 MB job, round 3.)
    auto zero_fill_slice = [&]() {
        if (!CKPT || zf.ptr == nullptr) return;
        const size_t base = (size_t)blockIdx.x * zf.per_block;
        for (uint32_t i = tid; i < zf.per_block; i += 256u)
            if (base + i < zf.n) { // non-temporal: the zeros must not push the splat rows / checkpoints out of the memory-side cache
                typedef float v4f __attribute__((ext_vector_type(4)));
                __builtin_nontemporal_store((v4f){0.f, 0.f, 0.f, 0.f}, reinterpret_cast<v4f *>(zf.ptr + base + i));
            }
    };

    if (a.masks != nullptr && !a.masks[tg.lin]) {
        if (inside) store_masked_pixel<CDIM>(a.render_colors, p.pix, CH, ch0, nch, bg);
        zero_fill_slice();
        return;
    }

    float qx0[4], qx1[4], qy0[4], qy1[4];
    bool qdone[4]; // block-uniform: quadrant finished (or empty)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const Rect r = wave_rect(a, tg, (uint32_t)q);
        qx0[q] = r.x0; qx1[q] = r.x1; qy0[q] = r.y0; qy1[q] = r.y1;
        qdone[q] = r.empty;
    }

    float T = 1.f, out[CDIM]; // T freezes at the stopping splat: it is the transmittance in front of it
    int32_t cur = 0;
    bool done = !inside;
#pragma unroll
    for (int k = 0; k < CDIM; ++k) out[k] = 0.f;

    const int32_t n = tg.range_end - tg.range_start;
    const int32_t base0 = tg.range_start & ~(GS_WAVE - 1);
    const int32_t num_batches = n > 0 ? (tg.range_end - base0 + BATCH - 1) / BATCH : 0;
    raise_priority_for(n);
    auto in_range = [&](int32_t idx) { return idx >= tg.range_start && idx < tg.range_end; };
    auto load_id = [&](int32_t idx) { return in_range(idx) ? a.flatten_ids[idx] : -1; };
    struct Staged {
        SplatRaw s;
        float col[CDIM];
    };
    auto gather = [&](int32_t g, Staged &o) {
        o.s.g = 0;
        o.s.mx = o.s.my = o.s.ca = o.s.cb = o.s.cc = o.s.opac = 0.f;
#pragma unroll
        for (int k = 0; k < CDIM; ++k) o.col[k] = 0.f;
        if (g >= 0) {
            if constexpr (WIDE) fetch_splat_wide<CDIM>(a, g, o.s, o.col, ch_off, cnt);
            else fetch_splat<CDIM>(a, g, o.s, o.col);
        }
    };
    int32_t id_cur = load_id(base0 + (int32_t)tid);
    int32_t id_nxt = load_id(base0 + BATCH + (int32_t)tid);
    Staged nxt;
    gather(id_cur, nxt);

    CkptCursor ck;
    ck.first(CKPT, tg.range_start, seg);
    // COST of every backward work item (tile, segment) = records this wave evaluated inside the segment: the backward's
    // work list is ordered by it, longest first (seg_items_sorted_kernel).  The tile's first segment reports into
    // cost_head[tile][wave]; a later segment k owns boundary k * seg and reports into cost_body[k][wave] -- written once
    // per (item, wave), no zero-fill and no atomics.
    uint32_t evals = 0;
    bool first_seg = true;
    auto store_cost = [&]() { // the segment in front of boundary ck.next_k has ended
        if (lane == 0 && cost_owner) {
            if (first_seg) cost_head[tg.lin * 4u + w] = evals;
            else {
                cost_body[(size_t)(ck.next_k - 1) * 4u + w] = evals;
                if (w == 0u) body_tile[ck.next_k - 1] = tg.lin; // the tile that owns boundary (ck.next_k - 1) * seg
            }
        }
        evals = 0;
        first_seg = false;
    };
    auto store_ckpt = [&]() {
        float *base = ckpt + (size_t)ck.next_k * (CH + 1) * 256;
        const uint32_t slot = w * 64u + lane;
        if (cost_owner) base[slot] = T;
#pragma unroll
        for (int k = 0; k < CDIM; ++k)
            if ((uint32_t)k < nch) base[(ch0 + k + 1) * 256 + slot] = out[k];
        store_cost();
    };

    // ---- the record walk of one (sub-batch, quadrant) list, shared by the cooperative and the solo path
#ifndef GS_WIDE_GW9
#define GS_WIDE_GW9 2
#endif
    constexpr int GW = WIDE ? (CDIM <= 9 ? GS_WIDE_GW9 : 2) : 4; // records per iteration of the bulk loop
    struct alignas(sizeof(list_t) * GW) Pack { list_t v[GW]; };
    // G records in one basic block (G = 4: the bulk of a list; G = 1: its last 1-3 records -- the lists used to be walked as
    // whole groups of four with their null-record padding, ~1.5 wasted evaluations per (sub-batch, quadrant) list = 9 % of
    // all evaluations; the padding is still written (harmless) but no longer walked)
    auto group = [&](auto gtag, const list_t *offs, uint32_t &cur_off) {
        constexpr int G = decltype(gtag)::value;
        float4 c0[G], c1[G];
        float c2x[G], c2y[G]; // colours 2, 3 (only what CDIM needs is read)
        float4 cw[G][WIDE ? NCW : 1]; // WIDE: colours 2 .. CDIM - 1
        uint32_t off[G];
        {
#pragma unroll
            for (int g = 0; g < G; ++g) off[g] = offs[g];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float4 *r = reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(s_rec) + off[g]);
                c0[g] = r[0];
                c1[g] = r[1];
                c2x[g] = c2y[g] = 0.f;
                if constexpr (WIDE) {
#pragma unroll
                    for (int j = 0; j < NCW; ++j) cw[g][j] = r[2 + j];
                }
                if (CDIM == 3) c2x[g] = reinterpret_cast<const float *>(r + 2)[0];
                if (CDIM == 4) {
                    const float2 v = reinterpret_cast<const float2 *>(r + 2)[0];
                    c2x[g] = v.x;
                    c2y[g] = v.y;
                }
            }
        }
        // The forward is ~80 % VALU-issue bound (every extra instruction per record costs ~6 us of the kernel, round 2):
        // the selects are merged (one for the alpha actually applied, one for the last contributor, both on the same
        // condition) and the conditions themselves combined on the scalar unit.
        float alpha[G];
        bool ok[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float dx = c0[g].x - px, dy = c0[g].y - py;
            SplatSample sm;
            ok[g] = splat_sample(dx, dy, c0[g].z, c0[g].w, c1[g].x, c1[g].y, sm);
            alpha[g] = sm.alpha;
        }
        // T is FROZEN at the stopping splat (= the transmittance in front of it, what the epilogue and the
        // checkpoints need), so a live pixel always has T > 1e-4 and a rejected record (a_eff = 0) cannot stop it
#pragma unroll
        for (int g = 0; g < G; ++g) {
            // exclusive stop: the record that would take T to <= 1e-4 is not composited and ends the pixel.  ONE
            // select (the alpha actually applied: 0 for a finished or finishing pixel) instead of separate selects
            // for the weight and for T -- T is then recomputed with it (a second fma is cheaper than a select)
            const float Tj = T;
            const bool stop = ok[g] && (__builtin_fmaf(-Tj, alpha[g], Tj) <= GS_T_MIN);
            done = done || stop;
            const bool use = ok[g] && !done; // composited: accepted, and the pixel neither finished nor finishing
            const float a_use = use ? alpha[g] : 0.f;
            const float vis = a_use * Tj;
            out[0] += c1[g].z * vis;
            if (CDIM > 1) out[CDIM > 1 ? 1 : 0] += c1[g].w * vis;
            if constexpr (WIDE) {
#pragma unroll
                for (int k = 2; k < CDIM; ++k) {
                    const float4 v = cw[g][(k - 2) / 4];
                    const int e = (k - 2) % 4;
                    out[k] += (e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w) * vis;
                }
            } else {
                if (CDIM > 2) out[CDIM > 2 ? 2 : 0] += c2x[g] * vis;
                if (CDIM > 3) out[CDIM > 3 ? 3 : 0] += c2y[g] * vis;
            }
            cur_off = use ? off[g] : cur_off;
            T = __builtin_fmaf(-Tj, a_use, Tj);
        }
    };
    auto walk = [&](const list_t *lst, const uint32_t cnt, uint32_t &cur_off) {
        // FOUR records per iteration, in one basic block: a lone wave issues one instruction per
        // ~5 cycles and a record is a ~25-deep dependent chain, so one record at a time costs
        // ~390 cycles (measured) against ~40 instructions x 5 cycles of issue.  The four alpha
        // evaluations are independent; only T <- T - T a (one fma) is carried from record to record.
        // The records come from the compacted list of this (sub-batch, quadrant): no bit scan, no validity flags.
        // (No explicit prefetch of the next group: it cost 40 VGPRs, i.e. two waves per SIMD, and the
        // kernel's duration is rounds of workgroups x their lifetime, not the walk of one list.)
        const uint32_t full = cnt & ~(uint32_t)(GW - 1);
        Pack pk_next = *reinterpret_cast<const Pack *>(lst); // GW record offsets, one broadcast read
        for (uint32_t j = 0; j < full; j += GW) {
            const Pack pk = pk_next;
            pk_next = *reinterpret_cast<const Pack *>(lst + j + GW); // next group's offsets (row is 72 long: in bounds)
            group(std::integral_constant<int, GW>{}, pk.v, cur_off);
        }
        for (uint32_t j = full; j < cnt; ++j) group(std::integral_constant<int, 1>{}, lst + j, cur_off);
    };

    // ---- SOLO path for the longest lists.  A tile's lifetime under the cooperative scheme is the sum over its batches
    // of the BUSIEST quadrant's work (the four waves meet at a barrier every 256 entries); the tiles with thousands of
    // entries run alone at the end of the kernel and set its duration.  There every wave walks the whole list by itself,
    // 64 entries at a time, culling against its own quadrant only: no barrier, its time is its own work, and a quadrant
    // that is done leaves.  (4x the gathers for these tiles -- 18 % of the pairs at config 2.)
    const bool solo = solo_min > 0 && n >= solo_min;
    if (solo) {
        float rx0 = qx0[0], ry0 = qy0[0];
#pragma unroll
        for (int q = 1; q < 4; ++q)
            if (w == (uint32_t)q) { rx0 = qx0[q]; ry0 = qy0[q]; }
        const int32_t n_sb = (tg.range_end - base0 + GS_WAVE - 1) / GS_WAVE;
        int32_t sid_cur = load_id(base0 + (int32_t)lane);
        int32_t sid_nxt = load_id(base0 + GS_WAVE + (int32_t)lane);
        Staged snx;
        gather(sid_cur, snx);
        __syncthreads(); // the null record (written by the first lanes of wave 0) is visible to every wave
        for (int32_t sbi = 0; sbi < n_sb; ++sbi) {
            const uint32_t buf = (uint32_t)sbi & (uint32_t)(NBUF - 1);
            const int32_t sb_start = base0 + sbi * GS_WAVE;
            const uint32_t slot = buf * BATCH + w * GS_WAVE + lane; // my record slot: the wave's own quarter of the buffer
            unsigned long long m;
            {
                const Staged st = snx;
                CullSplat cs;
                const bool live = sid_cur >= 0 && cull_prepare(st.s, cs);
                // cull against the bounding rectangle of the pixels that are still being composited (finished pixels ignore
                // every further record): the longest lists are walked to their end by a few unsaturated pixels
                const unsigned long long alive = __ballot(!done);
                bool touch = false;
                if (alive != 0ull) {
                    const LiveRect lr = live_rect(alive, rx0, ry0);
                    touch = live && rect_touch(st.s, cs, lr.x0, lr.x1, lr.y0, lr.y1);
                }
                m = __ballot(touch);
                if (touch) {
                    write_record<CDIM>(&s_rec[slot * REC], st.s, st.col);
                    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    s_list[buf][w][w][below] = (list_t)(slot * REC * 16u);
                }
                const uint32_t cnt = (uint32_t)__popcll(m);
                if (lane < 3u && cnt + lane < ((cnt + 3u) & ~3u)) s_list[buf][w][w][cnt + lane] = (list_t)NULL_REC_OFF;
            }
            sid_cur = sid_nxt;
            if (sbi + 1 < n_sb) gather(sid_cur, snx);
            sid_nxt = (sbi + 2 < n_sb) ? load_id(sb_start + 2 * GS_WAVE + (int32_t)lane) : -1;
            __builtin_amdgcn_wave_barrier(); // (LDS operations of one wave complete in order)
            if (CKPT) ck.before(sb_start, tg.range_end, seg, store_ckpt);
            if (m == 0ull) continue;
            uint32_t cur_off = 0xffffffffu;
            if (CKPT) evals += (uint32_t)__popcll(m);
            walk(&s_list[buf][w][w][0], (uint32_t)__popcll(m), cur_off);
            if (cur_off != 0xffffffffu) cur = sb_start + (int32_t)(record_index<REC>(cur_off >> 4) & 63u); // (slot & 63 = the staging lane)
            if (__all(done)) break;
        }
    } else
    for (int32_t b = 0; b < num_batches; ++b) {
        const uint32_t buf = (uint32_t)b & (uint32_t)(NBUF - 1);
        const int32_t batch_start = base0 + b * BATCH;
        // ---- stage: exact cull of my entry against the four quadrants
        {
            const Staged st = nxt;
            const bool have = id_cur >= 0;
            CullSplat cs;
            const bool live = have && cull_prepare(st.s, cs);
            unsigned long long m[4];
            bool any_touch = false;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                // (culling against the rectangle of the still-unfinished pixels, as the solo path does, was measured here too:
                // 0.210 -> 0.215 ms -- these tiles are short, the masks reach the staging threads two batches late)
                const bool touch = live && !qdone[q] && rect_touch(st.s, cs, qx0[q], qx1[q], qy0[q], qy1[q]);
                any_touch |= touch;
                m[q] = __ballot(touch);
            }
            if (any_touch) write_record<CDIM>(&s_rec[(buf * BATCH + tid) * REC], st.s, st.col);
            {
                // compacted lists: a lone wave issues one instruction per ~5 cycles WHATEVER its kind, so the consumer
                // must not spend a dozen scalar instructions per record on bit scans -- it reads ready-made offsets
                const uint32_t my_off = (buf * BATCH + tid) * REC * 16u;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m[q] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m[q], 0u));
                    if ((m[q] >> lane) & 1ull) s_list[buf][w][q][below] = (list_t)my_off;
                    const uint32_t cnt = (uint32_t)__popcll(m[q]);
                    if (lane < 3u && cnt + lane < ((cnt + 3u) & ~3u)) s_list[buf][w][q][cnt + lane] = (list_t)NULL_REC_OFF;
                }
            }
            const bool wave_done = __all(done); // evaluated by all 64 lanes, before the branch
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) s_mask[buf][w][q] = m[q];
                s_done[buf][w] = wave_done ? 1u : 0u;
            }
        }
        // ---- prefetch: splat data of the next batch (its ids are already here), ids of the one after
        id_cur = id_nxt;
        if (b + 1 < num_batches) gather(id_cur, nxt);
        id_nxt = (b + 2 < num_batches) ? load_id(batch_start + 2 * BATCH + (int32_t)tid) : -1;
        // LDS-only barrier: __syncthreads() would also drain vmcnt, i.e. wait for the gathers just issued
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        {
            const uint32_t d0 = s_done[buf][0], d1 = s_done[buf][1], d2 = s_done[buf][2], d3 = s_done[buf][3];
            if (d0 & d1 & d2 & d3) break; // every pixel of the tile is finished (block-uniform)
            qdone[0] = qdone[0] || d0; qdone[1] = qdone[1] || d1; qdone[2] = qdone[2] || d2; qdone[3] = qdone[3] || d3;
        }
        // ---- composite my quadrant over the four sub-batches
        uint32_t cur_off = 0xffffffffu; // record offset of the last contributor inside this batch (none yet)
#pragma unroll 1
        for (int sub = 0; sub < 4; ++sub) {
            const int32_t sb_start = batch_start + sub * GS_WAVE;
            if (sb_start >= tg.range_end) break;
            if (CKPT) ck.before(sb_start, tg.range_end, seg, store_ckpt);
            unsigned long long m = s_mask[buf][sub][w];
            m = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(m >> 32)) << 32) |
                (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)m); // (the builtin returns int: no sign extension)
            if (m == 0ull) continue;
            if (CKPT) evals += (uint32_t)__popcll(m);
            walk(&s_list[buf][sub][w][0], (uint32_t)__popcll(m), cur_off);
            if (__all(done)) break;
        }
        if (cur_off != 0xffffffffu) cur = batch_start + (int32_t)record_index<REC>((cur_off >> 4) - buf * (uint32_t)(BATCH * REC));
        if (NBUF == 1) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); // nobody restages while a wave still walks this batch
    }

    // The quadrant's last contributor: the maximum the backward takes over the same 64 last_ids (q_bin_max, -1 outside the image).
    // tile_last[tile][wave], stored like the costs; seg_items_build_kernel drops the segments behind the maximum of the four.
    const int32_t wave_last = __builtin_amdgcn_readfirstlane(wave_max_i32(inside ? cur : -1));
    if (CKPT && n > 0) {
        // boundaries after the last composited record (or after an early exit) carry the final state.  The backward restores a
        // quadrant from checkpoint k only in a segment k - 1 that holds one of the quadrant's contributors (q_live), so the planes
        // of the boundaries further back are not written: nobody reads this wave's quarter of them.  Their costs still are (the
        // build kernel's staleness check of body_tile depends on every boundary being reported in every call).
        while (ck.next_b < tg.range_end) {
            if (ck.next_b - seg <= wave_last) store_ckpt();
            else store_cost();
            ck.advance(seg);
        }
        store_cost(); // the tile's last segment
    }
    if (CKPT && cost_owner && lane == 0) tile_last[tg.lin * 4u + w] = wave_last;
    if (inside) store_pixel<CDIM>(a, p.pix, CH, ch0, nch, cost_owner, T, out, cur, bg);
    zero_fill_slice();
}

// The forward's workgroups in the order "longest list first": workgroup b composites tile order[b].  The hardware starts
// workgroups in index order, so the heavy tiles (up to ~7000 entries at BASELINE config 2 against 490 on average) begin at
// once instead of somewhere in the last rounds, where each of them used to hold the kernel's end back while the chip
// drained: raster_tile_fwd_kernel 197.5 -> 178.7 us (round 3; the same idea as the backward's cost-ordered work list).
// One workgroup: a counting sort of the tiles by list length in classes of 4 entries (2048 classes, the longest first; the
// order inside a class is whatever the atomics give -- it only decides which workgroup index a tile gets).
constexpr int ORDER_CLASSES = 2048, ORDER_THREADS = 1024, ORDER_PER = 8;
__global__ void __launch_bounds__(ORDER_THREADS) tile_order_kernel(uint32_t n_tiles_all, const int32_t *__restrict__ tile_offsets,
                                                                  uint32_t n_isects, uint32_t *__restrict__ order) {
    __shared__ uint32_t s_cnt[ORDER_CLASSES];
    __shared__ uint32_t s_wave[ORDER_THREADS / 64];
    const uint32_t tid = threadIdx.x;
    s_cnt[tid] = 0u;
    s_cnt[tid + ORDER_THREADS] = 0u;
    auto cls_of = [&](uint32_t t) {
        const uint32_t end = (t + 1u == n_tiles_all) ? n_isects : (uint32_t)tile_offsets[t + 1u];
        const uint32_t len = end - (uint32_t)tile_offsets[t];
        return (uint32_t)(ORDER_CLASSES - 1) - min(len >> 2, (uint32_t)(ORDER_CLASSES - 1)); // class 0 = the longest lists
    };
    // the first ORDER_PER x 1024 tiles keep their class in registers (all of them at 1080p: 8160 tiles)
    uint32_t cls[ORDER_PER];
#pragma unroll
    for (int k = 0; k < ORDER_PER; ++k) {
        const uint32_t t = (uint32_t)k * ORDER_THREADS + tid;
        cls[k] = t < n_tiles_all ? cls_of(t) : 0xffffffffu;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ORDER_PER; ++k)
        if (cls[k] != 0xffffffffu) atomicAdd(&s_cnt[cls[k]], 1u);
    for (uint32_t t = ORDER_PER * ORDER_THREADS + tid; t < n_tiles_all; t += ORDER_THREADS) atomicAdd(&s_cnt[cls_of(t)], 1u);
    __syncthreads();
    // exclusive scan of the class counts: two consecutive classes per thread
    const uint32_t c0 = s_cnt[2u * tid], c1 = s_cnt[2u * tid + 1u];
    uint32_t v = c0 + c1;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = __shfl_up(v, off, 64);
        if ((int)(tid & 63u) >= off) v += u;
    }
    if ((tid & 63u) == 63u) s_wave[tid >> 6] = v;
    __syncthreads();
    const uint32_t wv = (tid & 63u) < (uint32_t)(ORDER_THREADS / 64) ? s_wave[tid & 63u] : 0u; // the 16 wave totals, scanned by every wave
    uint32_t ws = wv;
#pragma unroll
    for (int off = 1; off < ORDER_THREADS / 64; off <<= 1) {
        const uint32_t u = __shfl_up(ws, off, 64);
        if ((int)(tid & 63u) >= off) ws += u;
    }
    const uint32_t base = __shfl(ws - wv, tid >> 6, 64); // exclusive total of the waves in front of mine
    const uint32_t excl = base + v - (c0 + c1);
    s_cnt[2u * tid] = excl; // (every thread rewrites exactly the two entries it read)
    s_cnt[2u * tid + 1u] = excl + c0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ORDER_PER; ++k)
        if (cls[k] != 0xffffffffu) order[atomicAdd(&s_cnt[cls[k]], 1u)] = (uint32_t)k * ORDER_THREADS + tid;
    for (uint32_t t = ORDER_PER * ORDER_THREADS + tid; t < n_tiles_all; t += ORDER_THREADS) order[atomicAdd(&s_cnt[cls_of(t)], 1u)] = t;
}

template <int CDIM>
void launch_tile_fwd(const RasterArgs &a, const RasterScratch &v, int32_t solo_min, ZeroFill zf, hipStream_t st, uint32_t ch_off, uint32_t cnt) {
    dim3 grid(a.C * a.tile_width * a.tile_height);
    if (v.ckpt != nullptr)
        hipLaunchKernelGGL((raster_tile_fwd_kernel<CDIM, true>), grid, dim3(256), 0, st, a, v.ckpt, v.seg, solo_min, v.cost_head, v.cost_body, v.body_tile, v.tile_last, v.class_count, zf, ch_off, cnt);
    else
        hipLaunchKernelGGL((raster_tile_fwd_kernel<CDIM, false>), grid, dim3(256), 0, st, a, v.ckpt, v.seg, solo_min, v.cost_head, v.cost_body, v.body_tile, v.tile_last, v.class_count, zf, ch_off, cnt);
}

// ---------------------------------------------------------------------------
// generic backward (no checkpoints, or more than 32 channels): one wave per quadrant of a tile, the whole list back to front
//   CMODE: 0 = colours in the LDS record (CDIM <= 4, v_out in registers)
//          1 = colours from global, v_out in registers (CDIM <= 32)
//          2 = any channel count: colours and v_out from global per splat (CDIM unused)
// record: R0, R1 as forward; R2 = (col2, col3, idx, g); R3 = (a, b, c, o)
// ---------------------------------------------------------------------------
template <int CDIM, int CMODE, bool ABS>
__global__ void __launch_bounds__(GS_WAVE) raster_wave_bwd_kernel(RasterArgs a, RasterGradArgs ga, uint32_t cnt, uint32_t ch_off, int use_v_alpha) {
    constexpr int REC = 4;
    constexpr int CR = (CMODE == 2) ? 1 : CDIM; // registers for v_out / colour sums
    __shared__ float4 s_rec[(GS_WAVE + 1) * REC];
    const uint32_t lane = threadIdx.x;
    const uint32_t lx = lane & 7u, ly = lane >> 3;
    const uint32_t vitem = xcd_remap(blockIdx.x, gridDim.x, a.xcd_group);
    const TileGeom tg = tile_geom(a, vitem >> 2);
    if (a.masks != nullptr && !a.masks[tg.lin]) return;
    const uint32_t q = vitem & 3u;
    const Rect rect = wave_rect(a, tg, q);
    if (rect.empty || tg.range_end <= tg.range_start) return;

    const float *bg = a.backgrounds ? a.backgrounds + (size_t)tg.cam * a.channels + ch_off : nullptr;
    // (not lane_pixel: an outside lane's pixel index is 0 here, and with the select behind the function every instance grows by 1 .. 8 instructions)
    const uint32_t ox = lx + 8u * (q & 1u), oy = ly + 8u * (q >> 1);
    const uint32_t x = tg.px0 + ox, y = tg.py0 + oy;
    const bool inside = ox < a.tile_size && oy < a.tile_size && x < a.image_width && y < a.image_height;
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    const size_t pix = inside ? ((size_t)tg.cam * a.image_height + y) * a.image_width + x : 0;
    const int64_t vpix = (int64_t)pix * ga.s_vrc_pix + (int64_t)ch_off * ga.s_vrc_ch; // the same pixel in v_render_colors (its own strides)
    const float T_final = inside ? 1.f - ga.render_alphas[pix] : 1.f;
    float T = T_final, Bq = 0.f, vc[CR];
    float bg_dot = 0.f;
    if (CMODE != 2) {
#pragma unroll
        for (int k = 0; k < CR; ++k) {
            vc[k] = (inside && (uint32_t)k < cnt) ? ga.v_render_colors[vpix + k * ga.s_vrc_ch] : 0.f;
            if (bg != nullptr && (uint32_t)k < cnt) bg_dot += bg[k] * vc[k];
        }
    } else {
        vc[0] = 0.f;
        if (bg != nullptr && inside)
            for (uint32_t k = 0; k < cnt; ++k) bg_dot += bg[k] * ga.v_render_colors[vpix + k * ga.s_vrc_ch];
    }
    const float v_a = (inside && use_v_alpha) ? ga.v_render_alphas[pix] : 0.f;
    const float Tw = T_final * (v_a - bg_dot);
    const int32_t bin_final = inside ? ga.last_ids[pix] : -1; // never matches
    const int32_t bin_max = wave_max_i32(max(-1, bin_final));
    if (bin_max < tg.range_start) return; // nothing was composited in this wave's pixels
    // nothing behind bin_max contributes: start there and walk back to front
    const int32_t first = min(tg.range_end - 1, bin_max);
    const int32_t total = first - tg.range_start + 1;
    const int32_t num_batches = (total + GS_WAVE - 1) / GS_WAVE;
    if (total >= HEAVY_TILE) __builtin_amdgcn_s_setprio(2);

    SplatRaw nxt = gather_splat(a, first - (int32_t)lane, first - (int32_t)lane >= tg.range_start);
    float ncol[CMODE == 0 ? CDIM : 1];
    if (CMODE == 0) {
#pragma unroll
        for (int k = 0; k < CDIM; ++k)
            ncol[k] = (first - (int32_t)lane >= tg.range_start && (uint32_t)k < cnt)
                          ? a.colors[(size_t)nxt.g * a.s_color + ch_off + k] : 0.f;
    }
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));

    for (int32_t b = 0; b < num_batches; ++b) {
        const int32_t batch_end = first - b * GS_WAVE; // lane l holds list index batch_end - l
        SplatRaw s = nxt;
        CullSplat cs;
        const int32_t my_idx = batch_end - (int32_t)lane;
        const bool live = (my_idx >= tg.range_start) && cull_prepare(s, cs) && rect_touch(s, cs, rect.x0, rect.x1, rect.y0, rect.y1);
        const unsigned long long lm = __ballot(live);
        const int count = __popcll(lm);
        if (live) {
            const int slot = __popcll(lm & lt_mask);
            float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
            if (CMODE == 0) {
                c0 = ncol[0];
                if (CDIM > 1) c1 = ncol[CDIM > 1 ? 1 : 0];
                if (CDIM > 2) c2 = ncol[CDIM > 2 ? 2 : 0];
                if (CDIM > 3) c3 = ncol[CDIM > 3 ? 3 : 0];
            }
            s_rec[slot * REC + 0] = make_float4(s.mx, s.my, -0.5f * LOG2E * s.ca, -LOG2E * s.cb);
            s_rec[slot * REC + 1] = make_float4(-0.5f * LOG2E * s.cc, __log2f(s.opac), c0, c1);
            s_rec[slot * REC + 2] = make_float4(c2, c3, __int_as_float(my_idx), __int_as_float(s.g));
            s_rec[slot * REC + 3] = make_float4(s.ca, s.cb, s.cc, s.opac);
        }
        if (b + 1 < num_batches) {
            const int32_t ni = first - (b + 1) * GS_WAVE - (int32_t)lane;
            nxt = gather_splat(a, ni, ni >= tg.range_start);
            if (CMODE == 0) {
#pragma unroll
                for (int k = 0; k < CDIM; ++k)
                    ncol[k] = (ni >= tg.range_start && (uint32_t)k < cnt) ? a.colors[(size_t)nxt.g * a.s_color + ch_off + k] : 0.f;
            }
        }
        __builtin_amdgcn_wave_barrier();

        float4 r0 = s_rec[0], r1 = s_rec[1], r2 = s_rec[2], r3 = s_rec[3];
        for (int j = 0; j < count; ++j) {
            const float4 c0 = r0, c1 = r1, c2 = r2, c3 = r3;
            r0 = s_rec[(j + 1) * REC + 0];
            r1 = s_rec[(j + 1) * REC + 1];
            r2 = s_rec[(j + 1) * REC + 2];
            r3 = s_rec[(j + 1) * REC + 3];
            const int32_t idx = __float_as_int(c2.z);
            const int32_t g = __float_as_int(c2.w);
            const float *cp = a.colors + (size_t)g * a.s_color + ch_off; // wave-uniform
            float col[CR];
            if (CMODE == 0) {
                col[0] = c1.z;
                if (CDIM > 1) col[CDIM > 1 ? 1 : 0] = c1.w;
                if (CDIM > 2) col[CDIM > 2 ? 2 : 0] = c2.x;
                if (CDIM > 3) col[CDIM > 3 ? 3 : 0] = c2.y;
            } else if (CMODE == 1) {
#pragma unroll
                for (int k = 0; k < CR; ++k) col[k] = (uint32_t)k < cnt ? cp[k] : 0.f;
            }
            float S0 = 0.f, Sx = 0.f, Sy = 0.f, Sxx = 0.f, Sxy = 0.f, Syy = 0.f, Ax = 0.f, Ay = 0.f;
            float Cs[CR];
#pragma unroll
            for (int k = 0; k < CR; ++k) Cs[k] = 0.f;
            const float dx = c0.x - px, dy = c0.y - py;
            SplatSample sm;
            const bool valid = splat_sample(dx, dy, c0.z, c0.w, c1.x, c1.y, sm, idx <= bin_final);
            const float araw = sm.araw, alpha = sm.alpha;
            const float ra = __builtin_amdgcn_rcpf(1.f - alpha);
            const float Tn = T * ra;
            const float facv = valid ? alpha * Tn : 0.f;
            float D = 0.f;
            if (CMODE == 2) {
                if (valid)
                    for (uint32_t k = 0; k < cnt; ++k) D += cp[k] * ga.v_render_colors[vpix + k * ga.s_vrc_ch];
            } else {
#pragma unroll
                for (int k = 0; k < CR; ++k) {
                    D += col[k] * vc[k];
                    Cs[k] += facv * vc[k];
                }
            }
            const float v_alpha = D * Tn + (Tw - Bq) * ra;
            // gradient gate: nothing for conic / xy / opacity when o * vis > GS_ALPHA_MAX (`&`: see seg_sample)
            const float v_sigma = (valid & (araw <= GS_ALPHA_MAX)) ? -araw * v_alpha : 0.f;
            Bq += facv * D;
            T = valid ? Tn : T;
            const float sdx = v_sigma * dx, sdy = v_sigma * dy;
            S0 += v_sigma;
            Sx += sdx;
            Sy += sdy;
            Sxx += sdx * dx;
            Sxy += sdx * dy;
            Syy += sdy * dy;
            if (ABS) {
                Ax += fabsf(c3.x * sdx + c3.y * sdy);
                Ay += fabsf(c3.y * sdx + c3.z * sdy);
            }
            if (!__any(valid)) continue;
            float *vcol = ga.v_colors + (size_t)g * ga.s_color + ch_off;
            if (CMODE == 2) {
                // any channel count: one reduction + atomic per channel
                for (uint32_t k = 0; k < cnt; ++k) {
                    // (0.f +: the sum used to start from zero -- one fma, a -0 product enters the reduction as +0)
                    const float c = wave_sum_lane63(0.f + facv * (inside ? ga.v_render_colors[vpix + k * ga.s_vrc_ch] : 0.f));
                    if (lane == GS_WAVE - 1) unsafeAtomicAdd(vcol + k, c); // (more than 4 channels: no deterministic mode, checked by the caller)
                }
            } else {
#pragma unroll
                for (int k = 0; k < CR; ++k) Cs[k] = wave_sum_lane63(Cs[k]);
            }
            S0 = wave_sum_lane63(S0);
            Sx = wave_sum_lane63(Sx);
            Sy = wave_sum_lane63(Sy);
            Sxx = wave_sum_lane63(Sxx);
            Sxy = wave_sum_lane63(Sxy);
            Syy = wave_sum_lane63(Syy);
            if (ABS) {
                Ax = wave_sum_lane63(Ax);
                Ay = wave_sum_lane63(Ay);
            }
            if (lane == GS_WAVE - 1) {
                const size_t gr = (size_t)g;
                if (CMODE != 2) {
#pragma unroll
                    for (int k = 0; k < CR; ++k)
                        if ((uint32_t)k < cnt) grad_add(ga, vcol + k, gr, 6u + ch_off + (uint32_t)k, Cs[k]);
                }
                grad_add(ga, ga.v_means2d + ga.s_xy * gr, gr, 0u, c3.x * Sx + c3.y * Sy);
                grad_add(ga, ga.v_means2d + ga.s_xy * gr + 1, gr, 1u, c3.y * Sx + c3.z * Sy);
                grad_add(ga, ga.v_conics + ga.s_conic * gr, gr, 2u, 0.5f * Sxx);
                grad_add(ga, ga.v_conics + ga.s_conic * gr + 1, gr, 3u, Sxy);
                grad_add(ga, ga.v_conics + ga.s_conic * gr + 2, gr, 4u, 0.5f * Syy);
                grad_add(ga, ga.v_opacities + ga.s_opac * gr, gr, 5u, -S0 / c3.w);
                if (ABS) {
                    grad_add(ga, ga.v_means2d_abs + ga.s_abs * gr, gr, 10u, Ax);
                    grad_add(ga, ga.v_means2d_abs + ga.s_abs * gr + 1, gr, 11u, Ay);
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// more than 4 channels (feature rendering): one quadrant per wave, colours read from global memory
template <int CDIM>
void launch_fwd(const RasterArgs &a, uint32_t cnt, uint32_t off, hipStream_t st) {
    dim3 grid(a.C * a.tile_width * a.tile_height * 4);
    hipLaunchKernelGGL((raster_wave_fwd_kernel<CDIM>), grid, dim3(GS_WAVE), 0, st, a, cnt, off);
}

template <int CDIM, int CMODE>
void launch_bwd(const RasterArgs &a, const RasterGradArgs &ga, uint32_t cnt, uint32_t off, int use_va, hipStream_t st) {
    dim3 grid(a.C * a.tile_width * a.tile_height * 4);
    if (ga.v_means2d_abs != nullptr)
        hipLaunchKernelGGL((raster_wave_bwd_kernel<CDIM, CMODE, true>), grid, dim3(GS_WAVE), 0, st, a, ga, cnt, off, use_va);
    else
        hipLaunchKernelGGL((raster_wave_bwd_kernel<CDIM, CMODE, false>), grid, dim3(GS_WAVE), 0, st, a, ga, cnt, off, use_va);
}

// ---------------------------------------------------------------------------
// Fast segmented backward for 1..4 channels (the hot case): one wave per (tile, segment) item,
// 4 pixels per lane.  Differences from the generic kernel above:
//   * no compaction: every lane stages its list entry at slot = lane, and FOUR ballots (one per
//     8x8 quadrant, ellipse-extent test against that quadrant) give four 64-bit SGPR masks.  The
//     walk iterates over the set bits of their union (s_ff1) and enters a quadrant's pixel code
//     through a scalar branch -- segments bound the critical path, so throughput is what
//     counts here, and a splat typically touches ~2 of the 4 quadrants;
//   * the 6 + CDIM (+2) per-splat sums are reduced by hand-scheduled interleaved v_add_f32_dpp
//     chains (dpp_reduce.h): 6 instructions per value, no moves, no hazards.
// Work-item lookup, gather, per-pixel state, batch staging, the sample body and the moments -> geometry gradients are the
// stages of rasterize_seg_dev.h, shared with raster_seg_bwd_wide_kernel (here over all CDIM channels, ChanAll); the walk
// (software-pipelined by two), the reductions and the grad_add layouts below are this kernel's own.
// record: R0 = (mx, my, a', b')  R1 = (c', log2 o, col0, col1)  R2 = (col2, col3, a, b)  R3 = (c, o, g, -)
// ---------------------------------------------------------------------------
#ifndef GS_SEG_WAVES
#define GS_SEG_WAVES 5
#endif
template <int CDIM, bool ABS, bool DET>
__global__ void __launch_bounds__(GS_WAVE, GS_SEG_WAVES) raster_seg_bwd_kernel(RasterArgs a, RasterGradArgs ga, int use_v_alpha, SegArgs sg) {
    constexpr int REC = 4;
    constexpr int ACC = 3; // float4 per accumulator slot: (Sx', Sy', Sxx, Sxy) (Syy, S0, C0, C1) (C2, C3, Ax, Ay)
    __shared__ float4 s_rec[GS_WAVE * REC];
    __shared__ float4 s_acc[GS_WAVE * ACC];
    const uint32_t lane = threadIdx.x;
    constexpr ChanAll<CDIM> ch{};
    TileGeom tg;
    int32_t seg_k;
    bool from_ckpt;
    if (!seg_item(a, sg, tg, seg_k, from_ckpt)) return;

    // issue the first batch's gathers before anything else: their latency overlaps the pixel-state
    // loads below.  The walk starts at the segment's far end; entries behind every pixel's
    // last_ids are dropped by the per-quadrant test (idx <= q_bin_max).
    const int32_t first = tg.range_end - 1;
    SplatRaw nxt;
    float ncol[CDIM];
    seg_fetch<CDIM>(a, first - (int32_t)lane, tg.range_start, ch, nxt, ncol);

    SegPixels<CDIM> px;
    seg_pixels_init<CDIM>(a, ga, use_v_alpha, sg, tg, seg_k, from_ckpt, ch, lane, px);
    if (px.q_live == 0u) return; // nothing composited in this segment for any pixel
    const int32_t total = first - tg.range_start + 1;
    const int32_t num_batches = (total + GS_WAVE - 1) / GS_WAVE;

    for (int32_t b = 0; b < num_batches; ++b) {
        const int32_t batch_end = first - b * GS_WAVE; // slot t holds list index batch_end - t
        unsigned long long qm[4];
        seg_stage<CDIM>(nxt, ncol, batch_end, tg.range_start, lane, px, qm, &s_rec[lane * REC]);
        if (b + 1 < num_batches) seg_fetch<CDIM>(a, first - (b + 1) * GS_WAVE - (int32_t)lane, tg.range_start, ch, nxt, ncol);
        __builtin_amdgcn_wave_barrier();

        unsigned long long any = qm[0] | qm[1] | qm[2] | qm[3];
        unsigned long long touched = 0ull; // slots whose sums were stored this batch
        // software pipeline: the next record is read from LDS while the current one is processed
        // (both compositing kernels are bound by the number of instructions a wave issues, scalar ones included -- round 2:
        // one dummy s_add per record costs as much as one dummy v_fma -- so the bookkeeping is kept on as few as possible)
        // The loop is unrolled by two with the roles of the two record register sets swapped (A current / B next, then B
        // current / A next): written as one set copied into the other, the copy was nine v_mov per record.
        struct Rec {
            float4 r0, r1, r2, r3;
        };
        auto load_rec = [&](int slot, Rec &r) {
            r.r0 = s_rec[slot * REC + 0];
            r.r1 = s_rec[slot * REC + 1];
            r.r2 = s_rec[slot * REC + 2];
            r.r3 = ABS ? s_rec[slot * REC + 3] : make_float4(0.f, 0.f, 0.f, 0.f);
        };
        auto next_slot = [&]() { return __builtin_ctzll(any | (1ull << 63)); }; // (an empty set prefetches slot 63: in bounds, never used)
        auto body = [&](const int t, const Rec &rec) {
            const float4 r0 = rec.r0, r1 = rec.r1, r2 = rec.r2, r3 = rec.r3;
            float col[CDIM];
            col[0] = r1.z;
            if (CDIM > 1) col[CDIM > 1 ? 1 : 0] = r1.w;
            if (CDIM > 2) col[CDIM > 2 ? 2 : 0] = r2.x;
            if (CDIM > 3) col[CDIM > 3 ? 3 : 0] = r2.y;
            const unsigned long long bit = 1ull << t;
            SegSums<CDIM> sm;
            seg_sample<CDIM, ABS>(r0, r1.x, r1.y, col, r2.z, r2.w, r3.x, batch_end - t, bit, qm, px, sm);
            if (!__any(sm.av_sum > 0.f)) return;
            // 8 values through the permlane butterfly (20 VALU), the rest through plain DPP chains.
            // slot floats: [Sx, Sy | Sxx, Sxy | Syy, S0 | C0, C1 | C2, C3, Ax, Ay]
            float lo, hi;
            const float C1v = CDIM > 1 ? sm.Cs[CDIM > 1 ? 1 : 0] : 0.f;
            float C2v = CDIM > 2 ? sm.Cs[CDIM > 2 ? 2 : 0] : 0.f, C3v = CDIM > 3 ? sm.Cs[CDIM > 3 ? 3 : 0] : 0.f;
            // RGB without absgrad (the hot case): the ninth sum rides in the row reduction of the butterfly and is stored as
            // its four row partials (added up at the flush, once per batch) -- 4 DPP adds instead of a chain of 6 with padding
            constexpr bool ROW3 = !ABS && CDIM == 3;
            if (ROW3) wave_reduce_sum_8_butterfly_rows(sm.Sx, sm.Syy, sm.Sxx, sm.Cs[0], sm.Sy, sm.S0, sm.Sxy, C1v, lo, hi, C2v);
            else wave_reduce_sum_8_butterfly(sm.Sx, sm.Syy, sm.Sxx, sm.Cs[0], sm.Sy, sm.S0, sm.Sxy, C1v, lo, hi);
            if (ROW3) {
            } else if (ABS) {
                if (CDIM > 3) wave_reduce_sum_4(C2v, C3v, sm.Ax, sm.Ay);
                else if (CDIM > 2) wave_reduce_sum_3(C2v, sm.Ax, sm.Ay);
                else wave_reduce_sum_2(sm.Ax, sm.Ay);
            } else {
                if (CDIM > 3) wave_reduce_sum_2(C2v, C3v);
                else if (CDIM > 2) wave_reduce_sum_1(C2v);
            }
            // park the totals in LDS; the atomics are issued once per batch by the lane that staged
            // the splat (full-width atomic instructions instead of 9 one-lane instructions per splat)
            touched |= bit;
            float *acc = reinterpret_cast<float *>(&s_acc[t * ACC]);
            if ((lane & 15u) == 15u) {
                const uint32_t row = lane >> 4; // rows 0..3 hold (v0,v4) (v2,v6) (v1,v5) (v3,v7)
                reinterpret_cast<float2 *>(acc)[row] = make_float2(lo, hi);
                if (ROW3) acc[8 + row] = C2v; // the four row partials of C2 in the slot's third float4
            }
            if (!ROW3 && lane == GS_WAVE - 1) s_acc[t * ACC + 2] = make_float4(C2v, C3v, sm.Ax, sm.Ay);
        };
        {
            Rec ra, rb;
            int ta = next_slot();
            load_rec(ta, ra);
            while (any) {
                any &= ~(1ull << ta); // (the same 1 << t serves the quadrant tests and the `touched` set)
                const int tb = next_slot();
                load_rec(tb, rb);
                body(ta, ra);
                if (!any) break;
                any &= ~(1ull << tb);
                ta = next_slot();
                load_rec(ta, ra);
                body(tb, rb);
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (ga.packed) {
            // Packed gradient rows [n_elems,16]: finalise per slot in LDS, then issue the atomics with
            // lane = (slot, component): the <= 12 components of a splat go out as ONE request to ONE
            // 64-byte line instead of 9-11 requests to 4 arrays (atomics were 27% of this kernel).
            if ((touched >> lane) & 1ull) {
                float4 a0 = s_acc[lane * ACC + 0], a1 = s_acc[lane * ACC + 1];
                seg_geom_grads(&s_rec[lane * REC], a0, a1.x, a1.y);
                // row layout: vx vy | ca cb cc | o | c0 c1 c2 c3 | ax ay   (a2 already holds c2 c3 ax ay)
                s_acc[lane * ACC + 0] = a0;
                s_acc[lane * ACC + 1] = a1;
                if (!ABS && CDIM == 3) { // C2 arrives as four row partials
                    const float4 a2 = s_acc[lane * ACC + 2];
                    reinterpret_cast<float *>(&s_acc[lane * ACC + 2])[0] = (a2.x + a2.y) + (a2.z + a2.w);
                }
            }
            __builtin_amdgcn_wave_barrier();
            const uint32_t sub = lane / 12u, comp = lane % 12u; // 5 slots x 12 components per instruction
            const bool comp_on = lane < 60u && (comp < 6u + (uint32_t)CDIM || (ABS && comp >= 10u));
            const float *accf = reinterpret_cast<const float *>(s_acc);
#pragma unroll 1
            for (uint32_t grp = 0; grp < 13u; ++grp) {
                if (((touched >> (grp * 5u)) & 0x1full) == 0ull) continue; // wave-uniform
                const uint32_t slot = grp * 5u + sub;
                if (comp_on && slot < 64u && ((touched >> slot) & 1ull)) {
                    const uint32_t g = (uint32_t)__float_as_int(s_rec[slot * REC + 3].z);
                    grad_add<DET ? 1 : 0>(ga, ga.v_means2d + (size_t)g * 16u + comp, (size_t)g, comp, accf[slot * (ACC * 4) + comp]);
                }
            }
        } else if ((touched >> lane) & 1ull) {
            float4 a0 = s_acc[lane * ACC + 0], a1 = s_acc[lane * ACC + 1];
            float4 a2 = s_acc[lane * ACC + 2];
            if (!ABS && CDIM == 3) a2.x = (a2.x + a2.y) + (a2.z + a2.w); // C2 arrives as four row partials
            // this lane staged slot `lane`: its raw conic / opacity / id are still in the record
            seg_geom_grads(&s_rec[lane * REC], a0, a1.x, a1.y);
            const size_t g = (size_t)__float_as_int(s_rec[lane * REC + 3].z);
            float *vcol = ga.v_colors + g * CDIM;
            grad_add<DET ? 1 : 0>(ga, vcol, g, 6u, a1.z);
            if (CDIM > 1) grad_add<DET ? 1 : 0>(ga, vcol + 1, g, 7u, a1.w);
            if (CDIM > 2) grad_add<DET ? 1 : 0>(ga, vcol + 2, g, 8u, a2.x);
            if (CDIM > 3) grad_add<DET ? 1 : 0>(ga, vcol + 3, g, 9u, a2.y);
            grad_add<DET ? 1 : 0>(ga, ga.v_means2d + ga.s_xy * g, g, 0u, a0.x);
            grad_add<DET ? 1 : 0>(ga, ga.v_means2d + ga.s_xy * g + 1, g, 1u, a0.y);
            grad_add<DET ? 1 : 0>(ga, ga.v_conics + ga.s_conic * g, g, 2u, a0.z);
            grad_add<DET ? 1 : 0>(ga, ga.v_conics + ga.s_conic * g + 1, g, 3u, a0.w);
            grad_add<DET ? 1 : 0>(ga, ga.v_conics + ga.s_conic * g + 2, g, 4u, a1.x);
            grad_add<DET ? 1 : 0>(ga, ga.v_opacities + ga.s_opac * g, g, 5u, a1.y);
            if (ABS) {
                grad_add<DET ? 1 : 0>(ga, ga.v_means2d_abs + ga.s_abs * g, g, 10u, a2.z);
                grad_add<DET ? 1 : 0>(ga, ga.v_means2d_abs + ga.s_abs * g + 1, g, 11u, a2.w);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// segmented launch: one wave per (tile, segment) item, 4 pixels per lane
template <int CDIM>
void launch_bwd_seg(const RasterArgs &a, const RasterGradArgs &ga, int use_va, const SegArgs &sg, hipStream_t st) {
    dim3 grid(sg.max_items, 1);
    const bool abs = ga.v_means2d_abs != nullptr, det = ga.det != nullptr;
    if (abs && det) hipLaunchKernelGGL((raster_seg_bwd_kernel<CDIM, true, true>), grid, dim3(GS_WAVE), 0, st, a, ga, use_va, sg);
    else if (abs) hipLaunchKernelGGL((raster_seg_bwd_kernel<CDIM, true, false>), grid, dim3(GS_WAVE), 0, st, a, ga, use_va, sg);
    else if (det) hipLaunchKernelGGL((raster_seg_bwd_kernel<CDIM, false, true>), grid, dim3(GS_WAVE), 0, st, a, ga, use_va, sg);
    else hipLaunchKernelGGL((raster_seg_bwd_kernel<CDIM, false, false>), grid, dim3(GS_WAVE), 0, st, a, ga, use_va, sg);
}

// Work list of the segmented backward, ORDERED BY COST, longest first.  Why: a (tile, segment) item lasts 20 ... 120 us
// (p10 ... max) and the hardware starts workgroups in index order, so with a list in arrival order the kernel ended with a
// ~95 us drain of long items at low occupancy; longest-first (LPT) leaves the short items for the end (measured: 365 -> 329 us).
// cost = what the forward counted for the item (records evaluated by the four quadrant waves).  Items are bucketed into
// COST_CLASSES classes, each with its own region of the item array and a counter (zeroed by the forward kernel); the
// backward maps its block index through the class counts, most expensive class first.  Built right after the forward
// kernel, inside gs_rasterize_fwd: the backward itself is ONE launch, and a repeated backward (retain_graph) reuses it.
//   unit u < n_tiles_all           : the first segment of tile u
//   unit u = n_tiles_all + k       : segment k of the tile that owns list boundary k * seg (body_tile[k], verified)
// A unit whose segment lies behind its tile's last contributor (tile_last, reported by the forward) is no item: 27 % of the
// units of BASELINE config 2, whose waves used to load their pixel state and leave (profiles/r25_dead_segments.txt).
// item = (tile, k, end, -): the walk covers list entries [max(range_start, k * seg), end).
__global__ void __launch_bounds__(GS_BLOCK) seg_items_build_kernel(uint32_t n_tiles_all, uint32_t n_isects, const int32_t *__restrict__ offsets,
                                                                   const uint8_t *__restrict__ masks, int32_t seg, uint32_t n_bounds,
                                                                   const uint32_t *__restrict__ cost_head, const uint32_t *__restrict__ cost_body,
                                                                   const uint32_t *__restrict__ body_tile, const int32_t *__restrict__ tile_last,
                                                                   uint32_t *__restrict__ class_count, uint4 *__restrict__ items, uint32_t max_items) {
    __shared__ uint32_t s_cnt[COST_CLASSES], s_base[COST_CLASSES];
    if (threadIdx.x < COST_CLASSES) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t u = blockIdx.x * GS_BLOCK + threadIdx.x;
    uint32_t tile = 0, cls = 0, local = 0;
    int32_t k = 0, end = 0;
    bool valid = false;
    auto range = [&](uint32_t t, int32_t &rs, int32_t &re) {
        rs = offsets[t];
        re = (t + 1 == n_tiles_all) ? (int32_t)n_isects : offsets[t + 1];
    };
    // Segment k of tile t (list [rs, re), segment start `start`) is an item only if the tile's last contributor (the maximum of
    // its four waves' tile_last = of its 256 last_ids) lies at or behind the segment's start: otherwise the backward's own test
    // q_bin_max[i] >= range_start fails for all four quadrants.  The item ends at the segment's end or right behind that last
    // contributor, whichever comes first.
    auto live = [&](uint32_t t, int32_t start, int32_t re) {
        const int4 l = reinterpret_cast<const int4 *>(tile_last)[t];
        const int32_t last = max(max(l.x, l.y), max(l.z, l.w));
        end = (int32_t)min(min((int64_t)re, ((int64_t)k + 1) * seg), (int64_t)last + 1);
        return last >= start;
    };
    if (u < n_tiles_all) {
        int32_t rs, re;
        range(u, rs, re);
        valid = re > rs && (masks == nullptr || masks[u]);
        tile = u;
        k = rs / seg;
        valid = valid && live(u, rs, re);
        if (valid) {
            const uint4 c = reinterpret_cast<const uint4 *>(cost_head)[u];
            cls = cost_class(c.x + c.y + c.z + c.w, seg);
        }
    } else if (u - n_tiles_all < n_bounds) {
        k = (int32_t)(u - n_tiles_all);
        const uint32_t t = body_tile[k]; // stale or never written unless boundary k * seg lies strictly inside a live tile
        if (k > 0 && t < n_tiles_all) {
            int32_t rs, re;
            range(t, rs, re);
            valid = (int64_t)rs < (int64_t)k * seg && (int64_t)k * seg < (int64_t)re && (masks == nullptr || masks[t]);
            tile = t;
            valid = valid && live(t, k * seg, re);
            if (valid) {
                const uint4 c = reinterpret_cast<const uint4 *>(cost_body)[k];
                cls = cost_class(c.x + c.y + c.z + c.w, seg);
            }
        }
    }
    if (valid) local = atomicAdd(&s_cnt[cls], 1u);
    __syncthreads();
    if (threadIdx.x < COST_CLASSES) {
        const uint32_t c = s_cnt[threadIdx.x];
        s_base[threadIdx.x] = c ? atomicAdd(&class_count[threadIdx.x], c) : 0u;
    }
    __syncthreads();
    if (valid) items[(size_t)cls * max_items + s_base[cls] + local] = make_uint4(tile, (uint32_t)k, (uint32_t)end, 0u);
}


// Deterministic mode, second pass: fixed-point sums -> the float gradient outputs (every row written: no zero-fill needed)
__global__ void __launch_bounds__(GS_BLOCK) raster_det_finalize_kernel(uint32_t n_elems, uint32_t channels, const long long *__restrict__ det,
                                                                       RasterGradArgs ga) {
    const uint32_t r = blockIdx.x * GS_BLOCK + threadIdx.x;
    if (r >= n_elems) return;
    const long long *d = det + (size_t)r * 24u;
    auto f = [&](uint32_t c) { return (float)((double)d[c] * GS_DET_INV_LO + (double)d[12u + c] * GS_DET_INV_HI); };
    ga.v_means2d[ga.s_xy * (size_t)r] = f(0);
    ga.v_means2d[ga.s_xy * (size_t)r + 1] = f(1);
    ga.v_conics[ga.s_conic * (size_t)r] = f(2);
    ga.v_conics[ga.s_conic * (size_t)r + 1] = f(3);
    ga.v_conics[ga.s_conic * (size_t)r + 2] = f(4);
    ga.v_opacities[ga.s_opac * (size_t)r] = f(5);
    for (uint32_t k = 0; k < channels; ++k) ga.v_colors[ga.s_color * (size_t)r + k] = f(6u + k);
    if (ga.v_means2d_abs != nullptr) {
        ga.v_means2d_abs[ga.s_abs * (size_t)r] = f(10);
        ga.v_means2d_abs[ga.s_abs * (size_t)r + 1] = f(11);
    }
}

} // namespace

// ---------------------------------------------------------------------------
// host side
// The SAME scratch buffer and the SAME plan must be handed to gs_rasterize_fwd and to the matching gs_rasterize_bwd, the
// buffer's contents preserved in between; its regions: RasterScratch (rasterize_common.h), laid out by scratch_view.
// ---------------------------------------------------------------------------
namespace {

// Tuning defaults = the measured optima on MI355X (profiles/round1_notes.md, round2_notes.md).  They travel in the
// caller's gs_raster_plan (gs_rasterize_plan): the library itself holds no tuning state.
//   seg        segment length of the depth-segmented backward in list entries (multiple of 64; 0: no segments,
//              the generic one-quadrant-per-wave backward runs instead).  256 since the work list is ordered
//              longest-first (round 2: 128 / 192 / 256 / 320 / 384 / 512 -> 0.338 / 0.317 / 0.305 / 0.312 / 0.324 /
//              0.331 ms backward, and half the checkpoint planes in the forward); with the list in arrival order
//              128 was best (round 1: 512 -> 1.14 ms, 256 -> 0.97 ms, 128 -> 0.89 ms).
//   solo_min   list length from which a tile's four forward waves stop cooperating (0: never). 2048.
//   xcd_fwd / xcd_bwd   work items per XCD group (xcd_remap).  16 tiles / 16 segment items.
constexpr uint32_t PLAN_MAGIC = 0x47535033u; // "GSP3"

// channel counts the tile forward / segmented backward cover: 1..4 in one launch, 5..16 in one launch of the wide instances,
// 17..32 as two launches over halves (rasterize_wide.hip)
constexpr uint32_t FAST_MAX_CHANNELS = 32;

// The forward route: the tile kernel wherever an instance covers the channel count -- the wide instances only under a
// caller's plan --, the generic kernel otherwise.
RasterRoute raster_route_fwd(uint32_t channels, const gs_raster_plan *plan) {
    if (channels <= 4u) return RasterRoute::TILE_NARROW;
    return (channels <= FAST_MAX_CHANNELS && plan != nullptr) ? RasterRoute::TILE_WIDE : RasterRoute::WAVE_GENERIC;
}

// Does the forward under this plan, handed the plan's scratch, leave checkpoints, costs and the work list behind?
bool plan_has_ckpt(const gs_raster_plan &p) { return p.seg > 0 && raster_route_fwd(p.channels, &p) != RasterRoute::WAVE_GENERIC; }

// The backward route: segmented only on top of what the forward of the SAME plan and scratch wrote (plan_has_ckpt) and the
// final render, on the kernels of the forward's route; the generic kernel otherwise.  The wide kernel has no deterministic
// mode, and absgrad is not linear in the image gradient: with it only what fits ONE launch goes the wide way.
RasterRoute raster_route_bwd(uint32_t channels, const gs_raster_plan *plan, const void *scratch, const float *render_colors,
                             const long long *det, bool absgrad) {
    if (plan == nullptr || scratch == nullptr || !plan_has_ckpt(*plan) || render_colors == nullptr) return RasterRoute::WAVE_GENERIC;
    const RasterRoute fwd = raster_route_fwd(channels, plan);
    if (fwd == RasterRoute::TILE_WIDE && (det != nullptr || (absgrad && raster_wide_chunk(channels) < channels)))
        return RasterRoute::WAVE_GENERIC;
    return fwd;
}

// The scratch of plan `p` as typed pointers (scratch == NULL: all NULL; the sizes hold either way)
RasterScratch scratch_view(const gs_raster_plan &p, void *scratch) {
    const bool ckpt = plan_has_ckpt(p), tile = raster_route_fwd(p.channels, &p) != RasterRoute::WAVE_GENERIC;
    size_t o = 256; // [0, 256): the class counters + padding; then the regions in this order, each padded to 256 bytes (tile_last: 16-byte loads)
    auto take = [&](bool on, size_t bytes) -> void * {
        void *r = (on && scratch != nullptr) ? (char *)scratch + o : nullptr;
        if (on) o += (bytes + 255) & ~(size_t)255;
        return r;
    };
    RasterScratch v;
    v.seg = p.seg;
    v.n_bounds = (ckpt ? p.n_isects / (uint32_t)p.seg : 0u) + 2u;
    v.max_items = p.n_tiles_all + v.n_bounds;
    v.class_count = (ckpt && scratch != nullptr) ? (uint32_t *)scratch : nullptr;
    v.items = (uint4 *)take(ckpt, (size_t)COST_CLASSES * v.max_items * sizeof(uint4));
    v.cost_head = (uint32_t *)take(true, (size_t)p.n_tiles_all * 4 * sizeof(uint32_t)); // (a region of every layout)
    if (!ckpt) v.cost_head = nullptr;
    v.cost_body = (uint32_t *)take(ckpt, (size_t)v.n_bounds * 4 * sizeof(uint32_t));
    v.body_tile = (uint32_t *)take(ckpt, (size_t)v.n_bounds * sizeof(uint32_t));
    v.tile_last = (int32_t *)take(ckpt, (size_t)p.n_tiles_all * 4 * sizeof(int32_t));
    v.ckpt = (float *)take(ckpt, (size_t)v.n_bounds * (p.channels + 1) * 256 * sizeof(float));
    v.tile_order = (uint32_t *)take(tile, (size_t)p.n_tiles_all * sizeof(uint32_t)); // heaviest lists first (tile_order_kernel)
    if (p.reserved[0] == 0u || p.n_tiles_all == 0u) v.tile_order = nullptr;
    v.total = o;
    return v;
}

} // namespace

int32_t raster_make_plan(uint32_t n_tiles_all, uint32_t n_isects, uint32_t channels, const int32_t *tuning, gs_raster_plan *plan) {
    memset(plan, 0, sizeof(*plan));
    // forward tiles longest list first: worth its one-workgroup ordering launch (10 us at 8 K tiles, 60 us at 65 K) while a batch has few
    // enough tiles for the tail to matter -- measured on BASELINE config 2's scene: +0.5 % at 1 camera, neutral at 2-3, -1.2 % at 4 and
    // -2.3 % at 8 cameras (32 K / 65 K tiles), so: up to three 1080p cameras' worth of tiles
    int32_t seg = 256, solo = 2048, xf = 16, xb = 16, order = n_tiles_all <= 24576u;
    if (tuning != nullptr) {
        if (tuning[0] >= 0) seg = ((tuning[0] + 63) / 64) * 64;
        if (tuning[1] >= 0) solo = tuning[1];
        if (tuning[2] >= 0) xf = tuning[2];
        if (tuning[3] >= 0) xb = tuning[3];
        if (tuning[4] >= 0) order = tuning[4] != 0;
    }
    // the segment length is doubled until the checkpoint array stays below 65536 boundaries (256 MB for RGB; the same
    // byte bound for more planes: 5..32 channels)
    while (seg > 0 && (uint64_t)n_isects / (uint32_t)seg * (channels > 4u ? channels + 1u : 4u) > 65536u * 4u) seg *= 2;
    plan->magic = PLAN_MAGIC;
    plan->n_tiles_all = n_tiles_all;
    plan->n_isects = n_isects;
    plan->channels = channels;
    plan->seg = seg;
    plan->solo_min = solo;
    plan->xcd_fwd = (uint32_t)xf;
    plan->xcd_bwd = (uint32_t)xb;
    plan->reserved[0] = (uint32_t)order; // forward: tiles with the longest lists first
    plan->scratch_bytes = scratch_view(*plan, nullptr).total;
    return 0;
}

bool raster_plan_ok(const gs_raster_plan *plan, uint32_t n_tiles_all, uint32_t n_isects, uint32_t channels) {
    return plan != nullptr && plan->magic == PLAN_MAGIC && plan->n_tiles_all == n_tiles_all && plan->n_isects == n_isects &&
           plan->channels == channels && plan->seg >= 0 && plan->seg % 64 == 0 &&
           plan->scratch_bytes == scratch_view(*plan, nullptr).total;
}

// the plan a call runs under: the caller's, or (no plan means no scratch) the default launch geometry without checkpoints
static gs_raster_plan plan_or_default(const RasterArgs &a, const gs_raster_plan *plan) {
    gs_raster_plan p;
    if (plan == nullptr) raster_make_plan(a.C * a.tile_width * a.tile_height, a.n_isects, a.channels, nullptr, &p);
    return plan != nullptr ? *plan : p;
}

int32_t raster_dispatch_fwd(const RasterArgs &a_in, const gs_raster_plan *plan, void *scratch, void *zero_fill, size_t zero_fill_bytes,
                            hipStream_t st) {
    RasterArgs a = a_in;
    const uint32_t n_tiles_all = a.C * a.tile_width * a.tile_height;
    const gs_raster_plan P = plan_or_default(a, plan);
    const RasterRoute route = raster_route_fwd(a.channels, plan);
    const RasterScratch v = scratch_view(P, scratch);
    // the side job: spread over the tile workgroups when each gets at most 256 KB of it, a plain fill otherwise
    ZeroFill zf = {nullptr, 0, 0u};
    if (zero_fill != nullptr && zero_fill_bytes > 0) {
        const size_t n16 = zero_fill_bytes / 16;
        const size_t per = (n16 + n_tiles_all - 1) / (n_tiles_all ? n_tiles_all : 1);
        const bool in_kernel = v.ckpt != nullptr && n_tiles_all > 0 && per <= 16384;
        if (in_kernel) zf = {(float4 *)zero_fill, n16, (uint32_t)per};
        else if (hipMemsetAsync(zero_fill, 0, zero_fill_bytes, st) != hipSuccess) { gs_set_error("rasterize: zero fill failed"); return 1; }
    }
    if (route == RasterRoute::WAVE_GENERIC) {
        // (no plan, or more than 32 channels) one quadrant per wave, exact chunks of 32 channels
        a.xcd_group = P.xcd_fwd * 4u;
        for (uint32_t off = 0; off < a.channels; off += 32) {
            uint32_t cnt = min(32u, a.channels - off);
            if (cnt <= 8) launch_fwd<8>(a, cnt, off, st);
            else if (cnt <= 16) launch_fwd<16>(a, cnt, off, st);
            else launch_fwd<32>(a, cnt, off, st);
        }
        return 0;
    }
    // one 256-thread workgroup per tile, the colours in the LDS record (5..32 channels, round 5: the wide instances, 17..32 as
    // two launches over halves); checkpoints for the segmented backward when the caller handed over scratch
    a.xcd_group = P.xcd_fwd;
    a.tile_order = v.tile_order;
    if (v.tile_order != nullptr)
        hipLaunchKernelGGL(tile_order_kernel, dim3(1), dim3(ORDER_THREADS), 0, st, n_tiles_all, a.tile_offsets, a.n_isects, v.tile_order);
    const uint32_t chunk = route == RasterRoute::TILE_NARROW ? a.channels : raster_wide_chunk(a.channels);
    for (uint32_t off = 0; off < a.channels; off += chunk) {
        const uint32_t cnt = min(chunk, a.channels - off);
        const ZeroFill z = off == 0u ? zf : ZeroFill{nullptr, 0, 0u};
        switch (route == RasterRoute::TILE_NARROW ? (int)cnt : raster_wide_instance(cnt)) {
            case 1: launch_tile_fwd<1>(a, v, P.solo_min, z, st, off, cnt); break;
            case 2: launch_tile_fwd<2>(a, v, P.solo_min, z, st, off, cnt); break;
            case 3: launch_tile_fwd<3>(a, v, P.solo_min, z, st, off, cnt); break;
            case 4: launch_tile_fwd<4>(a, v, P.solo_min, z, st, off, cnt); break;
            case 8: launch_tile_fwd<8>(a, v, P.solo_min, z, st, off, cnt); break;
            case 9: launch_tile_fwd<9>(a, v, P.solo_min, z, st, off, cnt); break;
            case 12: launch_tile_fwd<12>(a, v, P.solo_min, z, st, off, cnt); break;
            default: launch_tile_fwd<16>(a, v, P.solo_min, z, st, off, cnt); break;
        }
    }
    if (v.ckpt != nullptr) // the backward's work list, ordered by the costs just counted
        hipLaunchKernelGGL(seg_items_build_kernel, dim3(gs_div_up(v.max_items, GS_BLOCK)), dim3(GS_BLOCK), 0, st, n_tiles_all, a.n_isects,
                           a.tile_offsets, a.masks, v.seg, v.n_bounds, v.cost_head, v.cost_body, v.body_tile, v.tile_last, v.class_count, v.items, v.max_items);
    return 0;
}

int32_t raster_dispatch_bwd(const RasterArgs &a_in, const RasterGradArgs &ga, const float *render_colors, const gs_raster_plan *plan,
                            void *scratch, hipStream_t st) {
    RasterArgs a = a_in;
    const gs_raster_plan P = plan_or_default(a, plan);
    const int use_va = ga.v_render_alphas != nullptr;
    const uint32_t c = a.channels;
    const RasterRoute route = raster_route_bwd(c, plan, scratch, render_colors, ga.det, ga.v_means2d_abs != nullptr);
    if (route == RasterRoute::WAVE_GENERIC) {
        // no checkpoints (forward ran without scratch, or segments are switched off) or more than 32 channels:
        // one quadrant per wave walking the whole list back to front
        a.xcd_group = P.xcd_bwd * 4u;
        if (c == 1) launch_bwd<1, 0>(a, ga, 1, 0, use_va, st);
        else if (c == 2) launch_bwd<2, 0>(a, ga, 2, 0, use_va, st);
        else if (c == 3) launch_bwd<3, 0>(a, ga, 3, 0, use_va, st);
        else if (c == 4) launch_bwd<4, 0>(a, ga, 4, 0, use_va, st);
        else if (c <= 8) launch_bwd<8, 1>(a, ga, c, 0, use_va, st);
        else if (c <= 16) launch_bwd<16, 1>(a, ga, c, 0, use_va, st);
        else if (c <= 32) launch_bwd<32, 1>(a, ga, c, 0, use_va, st);
        else launch_bwd<1, 2>(a, ga, c, 0, use_va, st);
    } else {
        // depth-segmented, ONE launch per chunk: the work list was built by gs_rasterize_fwd (seg_items_build_kernel)
        const RasterScratch v = scratch_view(P, scratch);
        a.xcd_group = P.xcd_bwd;
        if (route == RasterRoute::TILE_WIDE) {
            raster_seg_bwd_wide(a, ga, use_va, v, render_colors, st);
        } else {
            const SegArgs sg = seg_args(v, render_colors);
            switch (c) {
                case 1: launch_bwd_seg<1>(a, ga, use_va, sg, st); break;
                case 2: launch_bwd_seg<2>(a, ga, use_va, sg, st); break;
                case 3: launch_bwd_seg<3>(a, ga, use_va, sg, st); break;
                default: launch_bwd_seg<4>(a, ga, use_va, sg, st); break;
            }
        }
    }
    if (ga.det != nullptr)
        hipLaunchKernelGGL(raster_det_finalize_kernel, dim3(gs_div_up(a.n_elems, GS_BLOCK)), dim3(GS_BLOCK), 0, st, a.n_elems, c, ga.det, ga);
    return 0;
}
