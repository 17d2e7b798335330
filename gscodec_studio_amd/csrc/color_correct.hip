// color_correct.hip -- the evaluation-time colour matching of examples/lib_bilagrid.py:56-126 (color_correct): per iteration one
// pass over the pixels that applies the previous warp and accumulates the masked normal equations of the next one
// (gs_color_correct_pass), and one small kernel that sums the per-workgroup records and solves them (gs_color_correct_solve).
// Everything is summed in double in a fixed order, without atomics: the result is bit-identical from run to run.
#include "gs_common.h"

namespace {

constexpr int cc_cols(int n) { return n * (n + 1) / 2 + n + 1; }
constexpr int cc_tri(int k) { return k * (k + 1) / 2; }
constexpr int cc_record(int n) { return cc_tri(cc_cols(n)) + cc_cols(n); }
constexpr int CC_RCOND_LOG2 = 40;  // eigenvalues at or below 2^-40 of the largest are null (gs_color_correct_rcond_log2)
constexpr int CC_SWEEPS = 20;  // Jacobi converges quadratically: 10 x 10 is done in 6 to 11 sweeps, the loop leaves then
static_assert(GS_BLOCK >= cc_record(3) && GS_BLOCK >= cc_cols(3) * cc_cols(3), "a thread per record entry and per matrix entry");

// the quadratic expansion of one pixel, in the reference's column order
template <int N>
GS_DEV void features(const float (&x)[N], double (&a)[cc_cols(N)]) {
    int k = 0;
#pragma unroll
    for (int c = 0; c < N; ++c)
#pragma unroll
        for (int d = c; d < N; ++d) a[k++] = (double)x[c] * (double)x[d];
#pragma unroll
    for (int c = 0; c < N; ++c) a[k++] = (double)x[c];
    a[k] = 1.0;
}

struct PassArgs {
    const float *x, *x0, *ref;
    int64_t x_stride, x0_stride;
    uint64_t P;
    float lo, hi;
    const double *warp;
    float *out;
    double *partials;
};

// grid (blocks, n, G): workgroup (b, c, g) walks the pixels of group g and owns channel c -- it writes column c of the applied
// image and the record of channel c's system, so a lane holds one record (at most 55 + 10 doubles), not n of them
template <int N, bool APPLY, bool ACC>
__global__ void __launch_bounds__(GS_BLOCK) color_correct_pass_kernel(PassArgs a) {
    constexpr int K = cc_cols(N), T = cc_tri(K), R = T + K;
    __shared__ double s_red[GS_BLOCK / GS_WAVE][ACC ? R : 1];
    const uint32_t c = blockIdx.y, g = blockIdx.z;
    const uint64_t base = (uint64_t)g * a.P;
    double w[APPLY ? K * N : 1];
    if (APPLY) {
#pragma unroll
        for (int i = 0; i < K * N; ++i) w[i] = a.warp[(size_t)g * (K * N) + i];
    }
    double acc[ACC ? R : 1];
#pragma unroll
    for (int i = 0; i < (ACC ? R : 1); ++i) acc[i] = 0.0;

    for (uint64_t p = (uint64_t)blockIdx.x * GS_BLOCK + threadIdx.x; p < a.P; p += (uint64_t)gridDim.x * GS_BLOCK) {
        const uint64_t e = base + p;
        float x[N];
#pragma unroll
        for (int d = 0; d < N; ++d) x[d] = a.x[e * a.x_stride + d];
        double f[K];
        if (APPLY) {
            features<N>(x, f);
#pragma unroll
            for (int d = 0; d < N; ++d) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < K; ++k) s += f[k] * w[k * N + d];
                // torch.clip: a NaN stays a NaN
                x[d] = (float)(s != s ? s : fmin(fmax(s, 0.0), 1.0));
            }
            a.out[e * N + c] = x[c];
        }
        if (ACC) {
            const float z0 = a.x0[e * a.x0_stride + c], b = a.ref[e * N + c];
            const bool keep = z0 >= a.lo && z0 <= a.hi && x[c] >= a.lo && x[c] <= a.hi && b >= a.lo && b <= a.hi;
            if (keep) {
                features<N>(x, f);
                int t = 0;
#pragma unroll
                for (int i = 0; i < K; ++i)
#pragma unroll
                    for (int j = i; j < K; ++j) acc[t++] += f[i] * f[j];
#pragma unroll
                for (int i = 0; i < K; ++i) acc[T + i] += f[i] * (double)b;
            }
        }
    }
    if (ACC) {
        const uint32_t wave = threadIdx.x / GS_WAVE;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const double s = wave_sum_f64(acc[i]);
            if (lane_id() == 0) s_red[wave][i] = s;
        }
        __syncthreads();
        if (threadIdx.x < R) {
            double s = 0.0;
#pragma unroll
            for (int v = 0; v < GS_BLOCK / GS_WAVE; ++v) s += s_red[v][threadIdx.x];
            a.partials[(((size_t)g * N + c) * gridDim.x + blockIdx.x) * R + threadIdx.x] = s;
        }
    }
}

// The Jacobi rotation of index i in a step that pairs it with `mate` (a mate >= K is a bye: the identity): the coefficients of
// rows i and mate of the old matrix in row i of the new one, J^T A J with J = [[c, s], [-s, c]] on the pair.  An off-diagonal
// entry below the rounding of its diagonal pair is left alone (|a_pq| <= sqrt(a_pp a_qq) in a positive semi-definite matrix).
template <int K>
GS_DEV bool rotation_of(const double (&a)[K][K + 1], int i, int mate, double &own, double &other) {
    own = 1.0;
    other = 0.0;
    if (mate >= K) return false;
    const int p = min(i, mate), q = max(i, mate);
    const double app = a[p][p], aqq = a[q][q], apq = a[p][q];
    if (!(fabs(apq) > 1e-22 * (fabs(app) + fabs(aqq)) && fabs(apq) > 1e-300)) return false;
    const double theta = (aqq - app) / (2.0 * apq);
    const double tn = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    own = 1.0 / sqrt(tn * tn + 1.0);
    other = i < mate ? -(tn * own) : tn * own;
    return true;
}

// grid (n, G), GS_BLOCK threads: one system per workgroup.  The four waves sum a quarter of the records each (b = wave, wave + 4,
// ... in ascending order), then the quarters are added in order.  The eigen-decomposition is the parallel-order cyclic Jacobi:
// a sweep is M - 1 steps (M = K rounded up to even) of a round-robin tournament, each step rotates K / 2 disjoint index pairs at
// once, and thread (i, j) of the first K K computes entry (i, j) of J^T A J (for i <= j, mirrored: the matrix stays exactly
// symmetric) and of V J from the old values -- reads, a barrier, writes, a barrier.
template <int N>
__global__ void __launch_bounds__(GS_BLOCK) color_correct_solve_kernel(const double *partials, uint32_t blocks, double *warp) {
    constexpr int K = cc_cols(N), T = cc_tri(K), R = T + K, M = K + (K & 1), WAVES = GS_BLOCK / GS_WAVE;
    __shared__ double s_part[WAVES][R];
    __shared__ double s_a[K][K + 1], s_v[K][K + 1], s_rhs[K], s_coef[K];
    __shared__ int s_bad, s_rotated[CC_SWEEPS];
    const uint32_t c = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
    const double *rec = partials + ((size_t)g * N + c) * blocks * R;
    if (t < CC_SWEEPS) s_rotated[t] = 0;
    if (t == 0) s_bad = 0;
    const uint32_t wave = t / GS_WAVE;
    for (uint32_t el = t % GS_WAVE; el < R; el += GS_WAVE) {
        double s = 0.0;
#pragma unroll 8
        for (uint32_t b = wave; b < blocks; b += WAVES) s += rec[(size_t)b * R + el];
        s_part[wave][el] = s;
    }
    __syncthreads();
    if (t < R) {
        double s = s_part[0][t];
#pragma unroll
        for (int v = 1; v < WAVES; ++v) s += s_part[v][t];
        if (!(fabs(s) <= 1.7976931348623157e308)) s_bad = 1;  // a NaN or an infinity among the sums: no solve (all write the same 1)
        s_part[0][t] = s;
    }
    __syncthreads();
    const bool bad = s_bad != 0, act = t < K * K;
    const int i = act ? (int)t / K : 0, j = act ? (int)t % K : 0;
    if (act) {
        const int r = min(i, j), q = max(i, j);
        s_a[i][j] = s_part[0][r * K - r * (r - 1) / 2 + (q - r)];  // the triangle is stored by rows
        s_v[i][j] = i == j ? 1.0 : 0.0;
        if (t < K) s_rhs[t] = s_part[0][T + t];
    }
    __syncthreads();
    if (!bad) {
        for (int sweep = 0; sweep < CC_SWEEPS; ++sweep) {
            for (int step = 0; step < M - 1; ++step) {
                // the circle method: index M - 1 stays, the others turn; the mate of i != step is 2 step - i (mod M - 1)
                auto mate_of = [&](int x) { return x == M - 1 ? step : x == step ? M - 1 : (2 * step - x + (M - 1)) % (M - 1); };
                double na = 0.0, nv = 0.0;
                bool ri = false, rj = false;
                if (act) {
                    const int mi = mate_of(i), mj = mate_of(j);
                    double ui, ti, uj, tj;
                    ri = rotation_of<K>(s_a, i, mi, ui, ti);
                    rj = rotation_of<K>(s_a, j, mj, uj, tj);
                    const int ki = mi < K ? mi : i, kj = mj < K ? mj : j;  // (a bye reads itself, times 0)
                    nv = s_v[i][j] * uj + s_v[i][kj] * tj;
                    if (i <= j) {
                        na = ui * (s_a[i][j] * uj + s_a[i][kj] * tj) + ti * (s_a[ki][j] * uj + s_a[ki][kj] * tj);
                        if (ri && j == mi) na = 0.0;  // the pivot: zero in exact arithmetic
                    }
                }
                __syncthreads();
                if (act) {
                    s_v[i][j] = nv;
                    if (i <= j) {
                        s_a[i][j] = na;
                        s_a[j][i] = na;
                    }
                    if (ri || rj) s_rotated[sweep] = 1;
                }
                __syncthreads();
            }
            if (!s_rotated[sweep]) break;  // the same in every thread
        }
    }
    // w = V diag(1 / lambda, or 0 at and below the cut) V^T A^T b
    double lmax = 0.0;
    for (int k = 0; k < K; ++k) lmax = fmax(lmax, s_a[k][k]);
    const double cut = lmax * (1.0 / (double)(1ull << CC_RCOND_LOG2));
    if (t < K) {
        const double lam = s_a[t][t];
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += s_v[k][t] * s_rhs[k];
        s_coef[t] = (!bad && lam > cut && lam > 0.0) ? s / lam : 0.0;
    }
    __syncthreads();
    if (t < K) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += s_v[t][k] * s_coef[k];
        warp[((size_t)g * K + t) * N + c] = s;
    }
}

template <int N>
void launch_pass(const PassArgs &a, dim3 grid, hipStream_t st) {
    if (a.warp && a.partials)
        hipLaunchKernelGGL((color_correct_pass_kernel<N, true, true>), grid, dim3(GS_BLOCK), 0, st, a);
    else if (a.warp)
        hipLaunchKernelGGL((color_correct_pass_kernel<N, true, false>), grid, dim3(GS_BLOCK), 0, st, a);
    else
        hipLaunchKernelGGL((color_correct_pass_kernel<N, false, true>), grid, dim3(GS_BLOCK), 0, st, a);
}

int32_t cc_shape(const char *fn, uint32_t G, uint32_t n, uint32_t blocks) {
    if (n < 1 || n > 3) {
        gs_set_error("%s: %u channels (1, 2 or 3 are supported)", fn, n);
        return 1;
    }
    if (G == 0) {
        gs_set_error("%s: no group (G = 0)", fn);
        return 1;
    }
    if (blocks == 0 || blocks > 65535u) {
        gs_set_error("%s: workgroup count %u (1 to 65535 per group and channel)", fn, blocks);
        return 1;
    }
    if ((uint64_t)blocks * n * G > 0x7fffffffull || G > 65535u) {
        gs_set_error("%s: %u groups of %u workgroups are more than the grid holds", fn, G, blocks);
        return 1;
    }
    return 0;
}

}  // namespace

extern "C" uint32_t gs_color_correct_rcond_log2(void) { return CC_RCOND_LOG2; }

extern "C" uint32_t gs_color_correct_record_doubles(uint32_t n) {
    return n == 1 ? cc_record(1) : n == 2 ? cc_record(2) : n == 3 ? cc_record(3) : 0;
}

extern "C" int32_t gs_color_correct_pass(const float *x, int64_t x_stride, const float *x0, int64_t x0_stride, const float *ref,
                                         uint32_t G, uint64_t P, uint32_t n, float lo, float hi, const double *warp, float *out,
                                         double *partials, uint32_t blocks, gs_stream_t stream) {
    if (cc_shape("gs_color_correct_pass", G, n, blocks)) return 1;
    GS_CHECK_ARG(x, "null pointer (x is required)");
    GS_CHECK_ARG(warp || partials, "null pointer: nothing to do (warp and partials both null)");
    GS_CHECK_ARG(!warp || out, "null pointer (out is required with warp)");
    GS_CHECK_ARG(!partials || (x0 && ref), "null pointer (x0 and ref are required with partials)");
    GS_CHECK_ARG(P > 0, "empty group (P = 0)");
    GS_CHECK_ARG(P <= 0x7fffffffull && (uint64_t)G * P <= 0x7fffffffull, "more than 2^31 - 1 pixels");
    GS_CHECK_ARG(x_stride >= (int64_t)n && (!partials || x0_stride >= (int64_t)n), "a pixel stride below the channel count");
    GS_CHECK_ARG((((uintptr_t)x | (uintptr_t)x0 | (uintptr_t)ref | (uintptr_t)out) % 4) == 0 &&
                     (((uintptr_t)warp | (uintptr_t)partials) % 8) == 0,
                 "misaligned pointer (floats need 4-byte, warp and partials 8-byte alignment)");
    GS_CHECK_ARG(!warp || out != x, "out must not be x (a workgroup reads every channel and writes one)");
    PassArgs a{x, x0, ref, x_stride, x0_stride, P, lo, hi, warp, out, partials};
    const dim3 grid(blocks, n, G);
    const hipStream_t st = (hipStream_t)stream;
    if (n == 1)
        launch_pass<1>(a, grid, st);
    else if (n == 2)
        launch_pass<2>(a, grid, st);
    else
        launch_pass<3>(a, grid, st);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int32_t gs_color_correct_solve(const double *partials, uint32_t G, uint32_t n, uint32_t blocks, double *warp,
                                          gs_stream_t stream) {
    if (cc_shape("gs_color_correct_solve", G, n, blocks)) return 1;
    GS_CHECK_ARG(partials && warp, "null pointer (partials and warp are required)");
    GS_CHECK_ARG((((uintptr_t)partials | (uintptr_t)warp) % 8) == 0, "misaligned pointer (partials and warp need 8-byte alignment)");
    const dim3 grid(n, G);
    const hipStream_t st = (hipStream_t)stream;
    if (n == 1)
        hipLaunchKernelGGL(color_correct_solve_kernel<1>, grid, dim3(GS_BLOCK), 0, st, partials, blocks, warp);
    else if (n == 2)
        hipLaunchKernelGGL(color_correct_solve_kernel<2>, grid, dim3(GS_BLOCK), 0, st, partials, blocks, warp);
    else
        hipLaunchKernelGGL(color_correct_solve_kernel<3>, grid, dim3(GS_BLOCK), 0, st, partials, blocks, warp);
    GS_CHECK_LAUNCH();
    return 0;
}
