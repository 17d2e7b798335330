// decode_act_dev.h -- what turns a trainer's raw parameters into rasterization()'s inputs (reference examples/simple_trainer.py:779-786:
// torch.exp on the log scales, torch.sigmoid on the opacity logits; F.normalize(dim=-1) on the quaternions), shared by the kernels
// that decode a file straight into those inputs: gs_decode_splats (codec.hip) and gs_ply_unpack (ply.hip).  No fma contraction
// (GS_FP_STRICT), so both kernels round alike whatever their translation unit is compiled with.  Device code only.
#pragma once
#include "gs_common.h"

namespace {

GS_DEV float decode_act_scale(float v) { return expf(v); }
GS_DEV float decode_act_opacity(float v) { GS_FP_STRICT; return 1.f / (1.f + expf(-v)); }

// F.normalize(dim=-1): x / max(||x||, 1e-12).  The sum of squares runs left to right: acc = q0 q0, then decode_sumsq(acc, q_i).
GS_DEV float decode_sumsq(float acc, float q) { GS_FP_STRICT; return acc + q * q; }
GS_DEV float decode_norm_divisor(float sumsq) { return fmaxf(sqrtf(sumsq), 1e-12f); }

} // namespace
