// ans_stream_dev.h -- ONE rANS STREAM, the layer under the coders of the on-disk formats (ans.hip: a static table per channel;
// gauss_ans.hip: a Gaussian per symbol; plane_codec.hip: a static table per scan diagonal).  Nothing here knows a model: a model hands in the frequency f and the cumulative frequency
// cum of a symbol at a probability resolution of 2^P (a plain value: it folds where it is a constant) and names the symbol of a slot.
//   state x: 32 bits, kept in [2^23, 2^31) between symbols
//   encode (f, cum):  while x >= f << (31 - P): emit x & 255, x >>= 8;   x = (x / f << P) + x % f + cum
//   decode:  slot = x & (2^P - 1), the model names s, f, cum;  x = f (x >> P) + slot - cum;  while x < 2^23: x = x << 8 | next byte
// Channel c of N symbols is cut into ceil(N / S) streams of S symbols and ONE LANE OWNS ONE STREAM: it walks its symbols backwards
// (the decoder reads forwards), fills a private worst-case slot (sized by the model's file) from the back and records length and final
// state; gs_ans_pack_slots (ans.hip) copies the slots into the dense payload.  The simplest shape whose output order the format fixes.
#pragma once
#include "gs_common.h"

namespace {

constexpr uint32_t ANS_L = 1u << 23, ANS_STATUS_SLOT_FULL = 2u; // bit 0 of an encoder's status word is its model's

// stream k of channel c: its first symbol within the channel, its length (S, or what is left of N), its id c n_streams + k
struct AnsStream { uint64_t begin; uint32_t len; uint64_t sid; };

GS_DEV AnsStream ans_stream(uint64_t N, uint32_t S, uint32_t k, uint32_t c, uint32_t n_streams) {
    const uint64_t begin = (uint64_t)k * S;
    return {begin, (uint32_t)(N - begin < (uint64_t)S ? N - begin : (uint64_t)S), (uint64_t)c * n_streams + k};
}

// renormalise, the bytes going to slot[--pos] (the order the decoder consumes them in), then code (f, cum), f >= 1
GS_DEV void ans_put(uint32_t &x, uint32_t f, uint32_t cum, uint32_t P, uint8_t *slot, uint32_t &pos, uint32_t &bad) {
    const uint32_t x_max = f << (31u - P);
    while (x >= x_max) {
        if (pos > 0u) slot[--pos] = (uint8_t)(x & 0xFFu);
        else bad |= ANS_STATUS_SLOT_FULL;
        x >>= 8;
    }
    const uint32_t q = x / f;
    x = (q << P) + (x - q * f) + cum;
}

GS_DEV void ans_finish(uint64_t sid, uint32_t len, uint32_t x, uint32_t bad, uint32_t *lengths, uint32_t *states, uint32_t *status) {
    lengths[sid] = len;
    states[sid] = x;
    if (bad != 0u) atomicOr(status, bad);
}

// a stream's bytes [rd, end), clamped into the payload, and the one at rd, 0 behind end: no read leaves [0, payload_bytes)
GS_DEV uint32_t ans_byte(const uint8_t *payload, uint64_t rd, uint64_t end) { return rd < end ? (uint32_t)payload[rd] : 0u; }

GS_DEV void ans_range(uint64_t payload_bytes, const int64_t *offsets, uint64_t sid, uint64_t &rd, uint64_t &end) {
    const int64_t o0 = offsets[sid], o1 = offsets[sid + 1];
    rd = o0 < 0 ? 0ull : ((uint64_t)o0 < payload_bytes ? (uint64_t)o0 : payload_bytes);
    end = o1 < 0 ? rd : ((uint64_t)o1 < rd ? rd : ((uint64_t)o1 < payload_bytes ? (uint64_t)o1 : payload_bytes));
}

// a valid stream needs at most two bytes here (x >= 2^(23 - P) after the step); a damaged one must not spin
GS_DEV uint32_t ans_advance(uint32_t x, uint32_t f, uint32_t cum, uint32_t slot, uint32_t P, const uint8_t *payload, uint64_t &rd, uint64_t end) {
    x = f * (x >> P) + slot - cum;
    for (uint32_t r = 0u; r < 2u && x < ANS_L; ++r, ++rd) x = (x << 8) | ans_byte(payload, rd, end);
    return x;
}

inline bool ans_shape_ok(uint64_t N, uint32_t C, uint32_t S, uint32_t P, uint32_t max_C, uint32_t min_P, uint32_t max_P) {
    return N >= 1 && N < (1ull << 32) && C >= 1 && C <= max_C && S >= 1 && S <= (1u << 24) && P >= min_P && P <= max_P;
}

} // namespace
