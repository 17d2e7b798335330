// rasterize_wide.hip -- R5b for 5..16 colour channels per launch (feature rendering: the 9-channel render of the reference's
// spacetime trainer, examples/simple_trainer_STG.py:531-551; 17..32 channels as two launches over halves): the depth-segmented
// backward of rasterize.hip (one wave64 per (tile, 256-entry segment) work item of the cost-ordered list, four pixels per lane,
// state restored from the forward's checkpoints, scalar B) with the colours in the LDS record.
//
// Replaces gsplat/cuda/csrc/rasterize_to_pixels_bwd.cu:17-277 for CDIM in {8, 9, 16, 17, 32} (the reference pads the channel
// count up to one of its template instances, gsplat/cuda/_wrapper.py:496-541); same per-pixel arithmetic and decisions as the
// 1..4-channel kernel (see the header of rasterize.hip).
//
// The stages both segmented backwards go through are ONE text, rasterize_seg_dev.h: work-item lookup, gather, per-pixel state,
// batch staging (culling, quadrant masks, R0..R3), the sample body and the moments -> geometry gradients.  This kernel runs them
// over the channel window of its launch (ChanWindow) and keeps what differs from raster_seg_bwd_kernel on purpose:
//   * the record's tail R4.. (col4 ...) behind the shared R0..R3, read back as wave-uniform scalars;
//   * the walk: a plain loop over the set bits, not the two-record software pipeline (the colour FMAs are independent work already);
//   * the 6 + CDIM (+ 2 with absgrad) per-splat sums go through butterflies of eight (wave_fold_8: two permlane-swap levels)
//     that share ONE interleaved row reduction (wave_rows_reduce_4 / _6), a tail of <= 4 values through plain DPP chains:
//     2.5 instructions per value instead of 6;
//   * gradients: the geometry (mean2d, conic, opacity, absgrad) into the packed 64-byte rows as before -- the projection
//     backward reads them in place --, the colours into their own dense [n_elems, channels] array, both with lane = (splat
//     slot, component) atomics (one request per splat and line);
//   * a launch covers channels [ch_off, ch_off + cnt): every gradient is LINEAR in the image gradient, so two launches over
//     the two halves of 17..32 channels add up exactly (v_render_alphas rides with the first).  absgrad is not linear: with it
//     more than 16 channels stay on the generic one-pass kernel (raster_route_bwd in rasterize.hip).  The launcher at the end,
//     raster_seg_bwd_wide, is called by raster_dispatch_bwd and shares raster_wide_chunk / raster_wide_instance with the forward.
#include "gs_common.h"
#include "rasterize_common.h"
#include "dpp_reduce.h"
#include "rasterize_seg_dev.h"

namespace {

// waves per SIMD the register allocation of the <= 9-channel instances is held to (0: the compiler's choice, 3 at 9 channels;
// 4 measured 1.072 -> 1.037 ms per 9-channel step at config 2, round 5)
#ifndef GS_WIDE_BWD_WAVES
#define GS_WIDE_BWD_WAVES 4
#endif
#ifndef GS_WIDE_BWD_WAVES_HI // the 12- / 16-channel instances (the compiler's choice: 161 / 189 VGPRs = 3 / 2 waves)
#define GS_WIDE_BWD_WAVES_HI 3 // (16 channels: 806 -> 723 us; 4 is out of reach: 13 KB of LDS per wave hold the CU to 12 waves)
#endif
template <int CDIM, bool ABS>
__global__ void __launch_bounds__(GS_WAVE, (GS_WIDE_BWD_WAVES > 0 && CDIM <= 9) ? GS_WIDE_BWD_WAVES : GS_WIDE_BWD_WAVES_HI) raster_seg_bwd_wide_kernel(RasterArgs a, RasterGradArgs ga, int use_v_alpha, SegArgs sg,
                                                                      uint32_t ch_off, uint32_t cnt) {
    static_assert(CDIM > 4 && CDIM <= 16, "5..16 channels per launch");
    constexpr int NC4 = (CDIM - 4 + 3) / 4; // float4s of colours 4..
    constexpr int REC = 4 + NC4;
    constexpr int NV = 6 + CDIM + (ABS ? 2 : 0); // per-splat sums
    constexpr int NGF = NV / 8, REM = NV % 8;    // full butterflies, tail
    constexpr bool TAIL_BFLY = REM > 4;          // tail as a zero-padded butterfly (else REM DPP chains)
    constexpr int NG = NGF + (TAIL_BFLY ? 1 : 0);
    static_assert(NG >= 2 && NG <= 3, "two or three butterflies");
    constexpr int ACCF = 8 * NG + ((!TAIL_BFLY && REM > 0) ? 4 : 0); // floats per accumulator slot
    // slot floats: [Sx Sy Sxx Sxy Syy S0 | C0 C1 C2 ... C(CDIM-1) | Ax Ay]: colour k at 6 + k, absgrad at 6 + CDIM
    // (after the flush's seg_geom_grads: [vx vy ca cb cc o | ...])
    __shared__ float4 s_rec[GS_WAVE * REC];
    __shared__ __attribute__((aligned(16))) float s_acc[GS_WAVE * ACCF];
    const uint32_t lane = threadIdx.x;
    const ChanWindow ch{ch_off, cnt, a.channels};
    TileGeom tg;
    int32_t seg_k;
    bool from_ckpt;
    if (!seg_item(a, sg, tg, seg_k, from_ckpt)) return;

    const int32_t first = tg.range_end - 1;
    SplatRaw nxt;
    float ncol[CDIM];
    seg_fetch<CDIM>(a, first - (int32_t)lane, tg.range_start, ch, nxt, ncol);

    SegPixels<CDIM> px;
    seg_pixels_init<CDIM>(a, ga, use_v_alpha, sg, tg, seg_k, from_ckpt, ch, lane, px);
    if (px.q_live == 0u) return;
    const int32_t total = first - tg.range_start + 1;
    const int32_t num_batches = (total + GS_WAVE - 1) / GS_WAVE;
    // colour atomics: lane = (slot sub, channel k), `per` slots per instruction
    const uint32_t per = 64u / cnt, csub = lane / cnt, ck = lane - csub * cnt;

    for (int32_t b = 0; b < num_batches; ++b) {
        const int32_t batch_end = first - b * GS_WAVE; // slot t holds list index batch_end - t
        unsigned long long qm[4];
        {
            float4 *rec = &s_rec[lane * REC];
            seg_stage<CDIM>(nxt, ncol, batch_end, tg.range_start, lane, px, qm, rec);
#pragma unroll
            for (int j = 0; j < NC4; ++j) {
                auto c = [&](int k) { return k < CDIM ? ncol[k < CDIM ? k : 0] : 0.f; };
                rec[4 + j] = make_float4(c(4 + 4 * j), c(5 + 4 * j), c(6 + 4 * j), c(7 + 4 * j));
            }
        }
        if (b + 1 < num_batches) seg_fetch<CDIM>(a, first - (b + 1) * GS_WAVE - (int32_t)lane, tg.range_start, ch, nxt, ncol);
        __builtin_amdgcn_wave_barrier();

        unsigned long long any = qm[0] | qm[1] | qm[2] | qm[3];
        unsigned long long touched = 0ull;
        while (any) {
            const int t = __builtin_ctzll(any);
            const unsigned long long bit = 1ull << t;
            any &= ~bit;
            const float4 *rec = &s_rec[t * REC];
            const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
            const float r3x = ABS ? reinterpret_cast<const float *>(rec + 3)[0] : 0.f;
            float col[CDIM];
            col[0] = r1.z; col[1] = r1.w; col[2] = r2.x; col[3] = r2.y;
#pragma unroll
            for (int j = 0; j < NC4; ++j) {
                const float4 v = rec[4 + j];
                if (4 + 4 * j < CDIM) col[4 + 4 * j < CDIM ? 4 + 4 * j : 0] = v.x;
                if (5 + 4 * j < CDIM) col[5 + 4 * j < CDIM ? 5 + 4 * j : 0] = v.y;
                if (6 + 4 * j < CDIM) col[6 + 4 * j < CDIM ? 6 + 4 * j : 0] = v.z;
                if (7 + 4 * j < CDIM) col[7 + 4 * j < CDIM ? 7 + 4 * j : 0] = v.w;
            }
            // the record is the same for every lane: the colours as wave-uniform SCALARS (one v_readfirstlane each) instead of 64 copies
            // in vector registers -- 9..16 VGPRs back, and with them every spill of these instances (224-408 bytes of scratch per lane
            // before, reloaded in this loop; 0 now): 16 channels 1.400 -> 1.375 ms per step, 9 channels 1.004 -> 0.994
#pragma unroll
            for (int k = 0; k < CDIM; ++k) col[k] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(col[k])));
            SegSums<CDIM> sm;
            seg_sample<CDIM, ABS>(r0, r1.x, r1.y, col, r2.z, r2.w, r3x, batch_end - t, bit, qm, px, sm);
            if (!__any(sm.av_sum > 0.f)) continue;
            // the value list behind the first butterfly: C2 .. C(CDIM-1) (, Ax, Ay), zero-padded
            auto L = [&](int i) -> float {
                if (i + 2 < CDIM) return sm.Cs[i + 2 < CDIM ? i + 2 : 0];
                if (ABS && i + 2 == CDIM) return sm.Ax;
                if (ABS && i + 2 == CDIM + 1) return sm.Ay;
                return 0.f;
            };
            float lo[3], hi[3];
            wave_fold_8(sm.Sx, sm.Syy, sm.Sxx, sm.Cs[0], sm.Sy, sm.S0, sm.Sxy, sm.Cs[1], lo[0], hi[0]);
            // group j >= 1 holds L[8(j-1) .. 8(j-1)+7]; fold arguments in the order that leaves them in list order in the slot
#pragma unroll
            for (int j = 1; j < NG; ++j) {
                const int o = 8 * (j - 1);
                wave_fold_8(L(o), L(o + 4), L(o + 2), L(o + 6), L(o + 1), L(o + 5), L(o + 3), L(o + 7), lo[j], hi[j]);
            }
            if (NG == 2) wave_rows_reduce_4(lo[0], hi[0], lo[1], hi[1]);
            else wave_rows_reduce_6(lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]);
            float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f; // the tail through plain chains (totals in lane 63)
            if (!TAIL_BFLY && REM > 0) {
                constexpr int o = 8 * (NGF - 1);
                t0 = L(o);
                if (REM > 1) t1 = L(o + 1);
                if (REM > 2) t2 = L(o + 2);
                if (REM > 3) t3 = L(o + 3);
                if (REM == 1) wave_reduce_sum_1(t0);
                else if (REM == 2) wave_reduce_sum_2(t0, t1);
                else if (REM == 3) wave_reduce_sum_3(t0, t1, t2);
                else wave_reduce_sum_4(t0, t1, t2, t3);
            }
            touched |= bit;
            float *acc = &s_acc[t * ACCF];
            if ((lane & 15u) == 15u) {
                const uint32_t row = lane >> 4; // rows 0..3 hold (v0,v4) (v2,v6) (v1,v5) (v3,v7) of every butterfly
#pragma unroll
                for (int j = 0; j < NG; ++j) reinterpret_cast<float2 *>(acc + 8 * j)[row] = make_float2(lo[j], hi[j]);
            }
            if (!TAIL_BFLY && REM > 0 && lane == GS_WAVE - 1) *reinterpret_cast<float4 *>(acc + 8 * NG) = make_float4(t0, t1, t2, t3);
        }
        __builtin_amdgcn_wave_barrier();
        // ---- flush.  Lane = slot: the moment sums become the geometry gradients in place
        if ((touched >> lane) & 1ull) {
            float *acc = &s_acc[lane * ACCF];
            float4 a0 = reinterpret_cast<const float4 *>(acc)[0];
            float2 a1 = reinterpret_cast<const float2 *>(acc)[2];
            seg_geom_grads(&s_rec[lane * REC], a0, a1.x, a1.y);
            reinterpret_cast<float4 *>(acc)[0] = a0;
            reinterpret_cast<float2 *>(acc)[2] = a1;
        }
        __builtin_amdgcn_wave_barrier();
        if (ga.packed) {
            // geometry into the packed rows: lane = (slot, component), 8 components per slot (0..5; 6, 7 = absgrad -> columns 10, 11)
            const uint32_t sub = lane >> 3, comp = lane & 7u;
            const bool comp_on = comp < 6u || ABS;
            const uint32_t src = comp < 6u ? comp : 6u + (uint32_t)CDIM + (comp - 6u), dst = comp < 6u ? comp : 4u + comp;
#pragma unroll 1
            for (uint32_t grp = 0; grp < 8u; ++grp) {
                if (((touched >> (grp * 8u)) & 0xffull) == 0ull) continue; // wave-uniform
                const uint32_t slot = grp * 8u + sub;
                if (comp_on && ((touched >> slot) & 1ull)) {
                    const uint32_t g = (uint32_t)__float_as_int(s_rec[slot * REC + 3].z);
                    unsafeAtomicAdd(ga.v_means2d + (size_t)g * 16u + dst, s_acc[slot * ACCF + src]);
                }
            }
        } else if ((touched >> lane) & 1ull) {
            const float *acc = &s_acc[lane * ACCF];
            const size_t g = (size_t)__float_as_int(s_rec[lane * REC + 3].z);
            unsafeAtomicAdd(ga.v_means2d + ga.s_xy * g, acc[0]);
            unsafeAtomicAdd(ga.v_means2d + ga.s_xy * g + 1, acc[1]);
            unsafeAtomicAdd(ga.v_conics + ga.s_conic * g, acc[2]);
            unsafeAtomicAdd(ga.v_conics + ga.s_conic * g + 1, acc[3]);
            unsafeAtomicAdd(ga.v_conics + ga.s_conic * g + 2, acc[4]);
            unsafeAtomicAdd(ga.v_opacities + ga.s_opac * g, acc[5]);
            if (ABS) {
                unsafeAtomicAdd(ga.v_means2d_abs + ga.s_abs * g, acc[6 + CDIM]);
                unsafeAtomicAdd(ga.v_means2d_abs + ga.s_abs * g + 1, acc[7 + CDIM]);
            }
        }
        // colours: lane = (slot, channel), `per` slots per instruction -- a splat's cnt floats are one contiguous request
#pragma unroll 1
        for (uint32_t s0 = 0; s0 < 64u; s0 += per) {
            if (((touched >> s0) & ((1ull << per) - 1ull)) == 0ull) continue; // wave-uniform
            const uint32_t slot = s0 + csub;
            if (csub < per && slot < 64u && ((touched >> slot) & 1ull)) {
                const size_t g = (size_t)__float_as_int(s_rec[slot * REC + 3].z);
                unsafeAtomicAdd(ga.v_colors + g * ga.s_color + ch_off + ck, s_acc[slot * ACCF + 6u + ck]);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

template <int CDIM>
void launch(const RasterArgs &a, const RasterGradArgs &ga, int use_va, const SegArgs &sg, uint32_t ch_off, uint32_t cnt, hipStream_t st) {
    if (ga.v_means2d_abs != nullptr)
        hipLaunchKernelGGL((raster_seg_bwd_wide_kernel<CDIM, true>), dim3(sg.max_items), dim3(GS_WAVE), 0, st, a, ga, use_va, sg, ch_off, cnt);
    else
        hipLaunchKernelGGL((raster_seg_bwd_wide_kernel<CDIM, false>), dim3(sg.max_items), dim3(GS_WAVE), 0, st, a, ga, use_va, sg, ch_off, cnt);
}

} // namespace

// The segmented backward of 5..32 channels from the forward's scratch (raster_dispatch_bwd, route TILE_WIDE): one launch per
// raster_wide_chunk of the channels, each on the instance that holds it (raster_wide_instance).  `use_va`: v_render_alphas
// takes part (it rides with the first launch only).
void raster_seg_bwd_wide(const RasterArgs &a, const RasterGradArgs &ga, int use_va, const RasterScratch &v, const float *render_colors,
                         hipStream_t st) {
    const SegArgs sg = seg_args(v, render_colors);
    const uint32_t chunk = raster_wide_chunk(a.channels);
    for (uint32_t off = 0; off < a.channels; off += chunk, use_va = 0) {
        const uint32_t cnt = min(chunk, a.channels - off);
        switch (raster_wide_instance(cnt)) {
            case 8: launch<8>(a, ga, use_va, sg, off, cnt, st); break;
            case 9: launch<9>(a, ga, use_va, sg, off, cnt, st); break;
            case 12: launch<12>(a, ga, use_va, sg, off, cnt, st); break;
            default: launch<16>(a, ga, use_va, sg, off, cnt, st); break;
        }
    }
}
