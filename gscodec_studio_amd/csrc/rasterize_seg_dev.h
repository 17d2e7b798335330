// rasterize_seg_dev.h -- the stages that the two depth-segmented compositing backwards share: raster_seg_bwd_kernel
// (rasterize.hip, 1..4 channels) and raster_seg_bwd_wide_kernel (rasterize_wide.hip, 5..16 channels per launch).  One wave64
// per (tile, segment) work item, lane (lx, ly) of an 8x8 grid owns one pixel in each 8x8 quadrant, slot t of a batch holds list
// entry batch_end - t.  In the order a kernel goes through them:
//   seg_item         block index -> work item, the tile's list range clamped to the segment
//   seg_fetch        one list entry's splat (zeros in front of the segment)
//   seg_pixels_init  the per-pixel state at the segment's far end (SegPixels), over a channel window
//   seg_stage        a batch: culling, the four quadrant masks, R0..R3 of the lane's record
//   seg_sample       one record against the lane's four pixels: the moment sums (SegSums)
//   seg_geom_grads   a slot's moment sums -> its geometry gradients
// What stays with each kernel, because it differs on purpose: the walk over a batch's records, the cross-lane reduction of the
// sums, the accumulator layout and the atomics.
// record: R0 = (mx, my, a', b')  R1 = (c', log2 o, col0, col1)  R2 = (col2, col3, a, b)  R3 = (c, o, g, -)  [wide: R4.. = col4 ...]
#pragma once

#include "rasterize_dev.h"

namespace {

// The channels [off, off + cnt) of an image with `stride` channels that one launch covers.  1..4 channels: the whole image, known
// at compile time (the `k < cnt` tests and the stride fold away); the wide kernel: its launch arguments.
template <int CDIM>
struct ChanAll {
    static constexpr uint32_t off = 0u, cnt = (uint32_t)CDIM, stride = (uint32_t)CDIM;
};
struct ChanWindow {
    uint32_t off, cnt, stride;
};

// Block index -> item: the classes in order of decreasing cost (the grid is an upper bound on the total).  False: nothing to do
// (behind the last item, or a masked tile).  tg comes back with its range clamped to the segment; from_ckpt: the segment ends
// in front of the tile's list end, i.e. the state at its far end is the forward's checkpoint seg_k + 1.
// The item carries its own end (it.z): the segment's, or, in the tile's last live segment, the entry behind the tile's last
// contributor -- everything behind that fails `my_idx <= q_bin_max[i]` in every quadrant (seg_stage), so the walk starts
// there, the state at the far end being the same as before (from_ckpt is taken from the unclamped segment).
GS_DEV bool seg_item(const RasterArgs &a, const SegArgs &sg, TileGeom &tg, int32_t &seg_k, bool &from_ckpt) {
    uint32_t n_work = 0;
#pragma unroll 8
    for (int c = 0; c < COST_CLASSES; ++c) n_work += sg.class_count[c];
    if (blockIdx.x >= n_work) return false;
    uint32_t r = xcd_remap(blockIdx.x, n_work, a.xcd_group);
    int cls = COST_CLASSES - 1;
    for (; cls > 0; --cls) {
        const uint32_t nc = sg.class_count[cls];
        if (r < nc) break;
        r -= nc;
    }
    const uint4 it = sg.items[(size_t)cls * sg.max_items + r];
    seg_k = (int32_t)it.y;
    tg = tile_geom(a, it.x);
    if (a.masks != nullptr && !a.masks[tg.lin]) return false;
    from_ckpt = (seg_k + 1) * sg.seg < tg.range_end;
    tg.range_start = max(tg.range_start, seg_k * sg.seg);
    tg.range_end = (int32_t)it.z;
    return true;
}

// The splat of list entry idx with the window's colours; zeros in front of the segment.
template <int CDIM, class Chan>
GS_DEV void seg_fetch(const RasterArgs &a, int32_t idx, int32_t range_start, const Chan &ch, SplatRaw &s, float *col) {
    s.g = 0;
    s.mx = s.my = s.ca = s.cb = s.cc = s.opac = 0.f;
#pragma unroll
    for (int k = 0; k < CDIM; ++k) col[k] = 0.f;
    if (idx >= range_start) {
        if constexpr (CDIM > 4) fetch_splat_wide<CDIM>(a, a.flatten_ids[idx], s, col, ch.off, ch.cnt);
        else fetch_splat<CDIM>(a, a.flatten_ids[idx], s, col);
    }
}

// A lane's four pixels (quadrant i: + 8 (i & 1), + 8 (i >> 1)) and the wave-uniform facts about the quadrants.
template <int CDIM>
struct SegPixels {
    float px0, py0;        // centre of the lane's pixel in quadrant 0
    float T[4];            // running transmittance
    float Wq[4];           // T_final (v_alpha_out - bg . v_out) - B  (the only way Tw and B are used)
    float vc[4][CDIM];     // v_render_colors of the window (zeros outside the image and behind cnt)
    int32_t bin_final[4];  // last contributor (-1 outside: never matches)
    int32_t q_bin_max[4];  // its maximum over the quadrant (SGPR)
    float qx0[4], qy0[4];  // first pixel centre of the quadrant (SGPR); no far corner: live_rect spans the pixels in play from here
    unsigned q_live;       // quadrants with a contributor inside the segment
};

// The state at the far end of segment seg_k of tile tg: the final render, or (from_ckpt) the forward's checkpoint seg_k + 1
// (T, accumulated colour): B = v_out . (colour_final - colour_ckpt).  q_live == 0 afterwards: nothing was composited in this
// segment for any pixel.  (The forward writes a quadrant's quarter of checkpoint seg_k + 1 only if the quadrant has a contributor
// at or behind the segment's start: a quadrant without its q_live bit may hold stale T / Wq here, which nothing reads.)
template <int CDIM, class Chan>
GS_DEV void seg_pixels_init(const RasterArgs &a, const RasterGradArgs &ga, int use_v_alpha, const SegArgs &sg, const TileGeom &tg,
                            int32_t seg_k, bool from_ckpt, const Chan &ch, uint32_t lane, SegPixels<CDIM> &p) {
    const uint32_t lx = lane & 7u, ly = lane >> 3;
    p.px0 = (float)(tg.px0 + lx) + 0.5f;
    p.py0 = (float)(tg.py0 + ly) + 0.5f;
    p.q_live = 0;
    const float *bg = a.backgrounds ? a.backgrounds + (size_t)tg.cam * a.channels + ch.off : nullptr;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t ox = lx + 8u * (i & 1), oy = ly + 8u * (i >> 1);
        const uint32_t x = tg.px0 + ox, y = tg.py0 + oy;
        const bool inside = ox < a.tile_size && oy < a.tile_size && x < a.image_width && y < a.image_height;
        const size_t pix = inside ? ((size_t)tg.cam * a.image_height + y) * a.image_width + x : 0;
        const float T_final = inside ? 1.f - ga.render_alphas[pix] : 1.f;
        p.T[i] = T_final;
        float bg_dot = 0.f;
#pragma unroll
        for (int k = 0; k < CDIM; ++k) {
            p.vc[i][k] = (inside && (uint32_t)k < ch.cnt) ? ga.v_render_colors[(int64_t)pix * ga.s_vrc_pix + (int64_t)(ch.off + k) * ga.s_vrc_ch] : 0.f;
            if (bg != nullptr && (uint32_t)k < ch.cnt) bg_dot += bg[k] * p.vc[i][k];
        }
        const float v_a = (inside && use_v_alpha) ? ga.v_render_alphas[pix] : 0.f;
        p.Wq[i] = T_final * (v_a - bg_dot);
        p.bin_final[i] = inside ? ga.last_ids[pix] : -1;
        if (from_ckpt && inside) {
            const float *cb = sg.ckpt + (size_t)(seg_k + 1) * (ch.stride + 1u) * 256 + i * 64 + lane; // planes [k][stride + 1][256]
            p.T[i] = cb[0];
            float bsum = 0.f;
#pragma unroll
            for (int k = 0; k < CDIM; ++k) {
                if ((uint32_t)k < ch.cnt) {
                    float fin = sg.render_colors[pix * ch.stride + ch.off + k];
                    if (bg != nullptr) fin -= T_final * bg[k];
                    bsum += p.vc[i][k] * (fin - cb[(ch.off + k + 1u) * 256u]);
                }
            }
            p.Wq[i] -= bsum;
        }
        p.q_bin_max[i] = __builtin_amdgcn_readfirstlane(wave_max_i32(p.bin_final[i])); // make it an SGPR
        if (p.q_bin_max[i] >= tg.range_start) p.q_live |= 1u << i;
        auto sgpr = [](float v) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v))); };
        p.qx0[i] = sgpr((float)(tg.px0 + 8u * (i & 1)) + 0.5f);
        p.qy0[i] = sgpr((float)(tg.py0 + 8u * (i >> 1)) + 0.5f);
    }
}

// One batch: lane stages the splat s (colours col) of list entry batch_end - lane at slot = lane.  No compaction: FOUR ballots
// (one per 8x8 quadrant) give four 64-bit SGPR masks qm of the slots that can touch the quadrant, and R0..R3 go to rec (the
// lane's record; a wide record's colour float4s follow behind).
// Pixels whose last contributor lies in front of this batch take no part in it (idx <= bin_final fails for every entry): the
// splats are culled against the bounding rectangle of the pixels that ARE still in play, not against the whole quadrant.  Most
// pixels saturate a third of the way into their tile's list, so towards the far end of a list a quadrant is often down to a
// handful of pixels.  Exact: a culled splat has alpha < 1/255 on every pixel that can use it.
template <int CDIM>
GS_DEV void seg_stage(const SplatRaw &s, const float *col, int32_t batch_end, int32_t range_start, uint32_t lane, const SegPixels<CDIM> &p,
                      unsigned long long (&qm)[4], float4 *rec) {
    CullSplat cs;
    const int32_t my_idx = batch_end - (int32_t)lane;
    const bool live = (my_idx >= range_start) && cull_prepare(s, cs);
    const int32_t batch_lo = max(range_start, batch_end - (GS_WAVE - 1));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned long long in_play = __ballot(p.bin_final[i] >= batch_lo);
        qm[i] = 0ull;
        if (((p.q_live >> i) & 1u) && in_play != 0ull) { // (wave-uniform)
            const LiveRect lr = live_rect(in_play, p.qx0[i], p.qy0[i]);
            const bool touch = live && (my_idx <= p.q_bin_max[i]) && rect_touch(s, cs, lr.x0, lr.x1, lr.y0, lr.y1);
            qm[i] = __ballot(touch);
        }
    }
    auto c = [&](int k) { return k < CDIM ? col[k < CDIM ? k : 0] : 0.f; };
    rec[0] = make_float4(s.mx, s.my, -0.5f * LOG2E * s.ca, -LOG2E * s.cb);
    rec[1] = make_float4(-0.5f * LOG2E * s.cc, __log2f(s.opac), c(0), c(1));
    rec[2] = make_float4(c(2), c(3), s.ca, s.cb);
    rec[3] = make_float4(s.cc, s.opac, __int_as_float(s.g), 0.f);
}

// What a lane sums over its pixels for one record: S0 = sum v_sigma, Sx = sum v_sigma dx, ... and C_k = sum fac v_out_k (the
// header of rasterize.hip); Ax, Ay: the absgrad sums; av_sum > 0 in the lanes with a valid sample in some quadrant (one add per
// pass; a lane-mask "or" costs four scalar instructions per pass).
template <int CDIM>
struct SegSums {
    float S0, Sx, Sy, Sxx, Sxy, Syy, Ax, Ay, Cs[CDIM], av_sum;
};

// The record of slot `bit` (list entry idx; r0, c' and log2 o as staged, colours col, the raw conic (e_ca, e_cb, e_cc) for
// absgrad) against the lane's pixel in every quadrant whose mask has the slot: steps T and Wq one splat towards the eye and
// returns the sums.
template <int CDIM, bool ABS>
GS_DEV void seg_sample(const float4 &r0, float qc, float lo2, const float (&col)[CDIM], float e_ca, float e_cb, float e_cc, int32_t idx,
                       unsigned long long bit, const unsigned long long (&qm)[4], SegPixels<CDIM> &p, SegSums<CDIM> &o) {
    o.S0 = o.Sx = o.Sy = o.Sxx = o.Sxy = o.Syy = o.Ax = o.Ay = o.av_sum = 0.f;
#pragma unroll
    for (int k = 0; k < CDIM; ++k) o.Cs[k] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (!(qm[i] & bit)) continue; // wave-uniform (scalar) branch
        const float dx = r0.x - (p.px0 + 8.f * (float)(i & 1)), dy = r0.y - (p.py0 + 8.f * (float)(i >> 1));
        SplatSample sm;
        const bool valid = splat_sample(dx, dy, r0.z, r0.w, qc, lo2, sm, idx <= p.bin_final[i]);
        // a rejected record gets alpha = 0: then ra = rcp(1) = 1 exactly, Tn = T and facv = 0, i.e. the
        // transmittance and the colour sums need no select of their own (selects cost 1.5 issue units here)
        const float av = valid ? sm.alpha : 0.f;
        o.av_sum += av;
        const float ra = __builtin_amdgcn_rcpf(1.f - av);
        const float Tn = p.T[i] * ra;
        const float facv = av * Tn;
        float D = 0.f;
#pragma unroll
        for (int k = 0; k < CDIM; ++k) {
            D += col[k] * p.vc[i][k];
            o.Cs[k] += facv * p.vc[i][k];
        }
        const float v_alpha = D * Tn + p.Wq[i] * ra;
        // gradient gate: nothing for conic / xy / opacity when o * vis > GS_ALPHA_MAX.  (`&`: two plain compares.  As `&&` the
        // condition reaches the code generator as a select, which costs this loop a v_max canonicalisation of araw per sample.)
        const float v_sigma = (valid & (sm.araw <= GS_ALPHA_MAX)) ? -sm.araw * v_alpha : 0.f;
        p.Wq[i] -= facv * D;
        p.T[i] = Tn;
        const float sdx = v_sigma * dx, sdy = v_sigma * dy;
        o.S0 += v_sigma;
        o.Sx += sdx;
        o.Sy += sdy;
        o.Sxx += sdx * dx;
        o.Sxy += sdx * dy;
        o.Syy += sdy * dy;
        if (ABS) {
            o.Ax += fabsf(e_ca * sdx + e_cb * sdy);
            o.Ay += fabsf(e_cb * sdx + e_cc * sdy);
        }
    }
}

// A slot's reduced moment sums m0 = (Sx, Sy, Sxx, Sxy), (m1x, m1y) = (Syy, S0) -> its geometry gradients
// (v_x, v_y, v_conic a, v_conic b), (v_conic c, v_opacity): v_xy = (a Sx + b Sy, b Sx + c Sy), v_conic = (Sxx/2, Sxy, Syy/2),
// v_opacity = -S0 / o, with the raw conic and opacity from R2, R3 of the slot's record.
GS_DEV void seg_geom_grads(const float4 *rec, float4 &m0, float &m1x, float &m1y) {
    const float4 e2 = rec[2], e3 = rec[3];
    const float e_ca = e2.z, e_cb = e2.w, e_cc = e3.x, e_op = e3.y;
    m0 = make_float4(e_ca * m0.x + e_cb * m0.y, e_cb * m0.x + e_cc * m0.y, 0.5f * m0.z, m0.w);
    m1x = 0.5f * m1x;
    m1y = -m1y / e_op;
}

} // namespace
