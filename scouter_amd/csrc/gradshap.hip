// GradientSHAP / expected gradients (Lundberg & Lee 2017; Erion et al. 2019; captum's GradientShap and LayerGradientShap of the
// reference's captum_vis.py; tools/attribution.py gradient_shap / layer_gradient_shap): the one gradient method here that explains
// against a BANK of baselines.  Every row of a batch walks from its own randomly drawn baseline by its own random fraction,
// optionally from a noisy copy of the image, and the gradients are summed times each row's own difference, which is regenerated
// from the draws and never stored.  Three streaming kernels, no atomics, no partial sums, one fixed order per output element.
//
// E is the flat element count of one image (or of one image's features), e the flat index, bank fp32 [R][E].
//
// The draws of sample s: (r0, r1, ., .) = Philox4x32-10 of the counter (0, s, 2, 0) under the key (seed_lo, seed_hi);
//   pick_s = ((uint64) r0 * R) >> 32, alpha_s = pg_uniform(r1).  The third counter word separates the streams: 0 is the normal
//   stream of noise_images, 1 the uniform stream of fidelity.hip, 2 this one.  A draw is a function of kernel arguments and the
//   sample's index only.  The two streaming kernels form the draws of up to 64 consecutive samples at once, lane l of a wave
//   that of sample (base + l), and read the one they need back with a lane read (gs_lane_pick / gs_lane_alpha): the pick, and the bank row it
//   selects, are uniform over the wave, and one vector Philox call serves 64 samples where a scalar one per sample sat in front
//   of every load (measured: 2.1 - 2.5 times the time of grad_accumulate with scalar draws).  Every lane of a wave must be
//   active for this (the invariant stated at gs_lane_pick): a thread past E works on group 0 and stores nothing.
// The noisy image: sigma == 0: x~_s = x, no Philox call, a -0.0 stays -0.0; sigma > 0: x~_s[e] = fmaf(sigma, z(seed, s, e), x[e]),
//   the expression and the counter (e / 4, s, 0, 0) of noise_images_kernel (ib_noise forms the same words).
// The row: d_s = x~_s - b_pick (one fp32 subtraction), row_s = fmaf(alpha_s, d_s, b_pick), the expression of path_images_kernel.
//
// gradshap_draws_kernel: picks[j], alphas[j] of the samples first + j, one thread per sample.
// gradshap_images_kernel: out[j] = row_{first + j}.  A thread owns the group of elements 4q .. 4q + 3 -- one Philox call serves
//   them -- for GS_JT values of j (blockIdx.y tiles j); the image's elements are loaded once.
// gradshap_accumulate_kernel: acc[e] = fma((double)g[j][e] * (double)d_{first + j}[e], inv_n, acc[e]) for j ascending, the
//   accumulators of the thread's group in registers over the whole loop.  The product is exact in fp64 (24 + 24 bits).
//
// Each kernel has a 16-byte form (E a multiple of 4 and every pointer 16-byte aligned) and a one-element form for everything else,
// the last group cut at E; the arithmetic of an element is one inlined expression shared by both, so they give the same bits.
#include "attr_common.h"

constexpr int GS_THREADS = 256;
constexpr int GS_JT = 8;                      // rows of a chunk per thread (gradshap_images): the image's elements are shared
constexpr int GS_ROWS = 8;                    // gradient rows (and their bank rows) a thread of gradshap_accumulate has in flight

// the draws of sample s against a bank of R baselines
__device__ __forceinline__ void gs_draw(unsigned seed_lo, unsigned seed_hi, unsigned s, int R, int& pick, float& alpha) {
    unsigned r[4];
    pg_philox(0u, s, 2u, 0u, seed_lo, seed_hi, r);
    pick = (int)(((unsigned long long)r[0] * (unsigned long long)(unsigned)R) >> 32);
    alpha = pg_uniform(r[1]);
}

// The pick / the fraction that lane `lane` of this wave holds in pick_v / alpha_v, as wave-uniform values.
// INVARIANT of gradshap_images_kernel and gradshap_accumulate_kernel: EVERY lane of the wave is active at the gs_draw that fills
// pick_v / alpha_v and at every lane read -- a lane read returns whatever an inactive lane's register holds.  So neither kernel
// may return early or branch on a per-thread condition before its last lane read: a thread past E is kept (`valid`), works on
// group 0 and stores nothing.
__device__ __forceinline__ int gs_lane_pick(int pick_v, int lane) { return __builtin_amdgcn_readlane(pick_v, lane); }
__device__ __forceinline__ float gs_lane_alpha(float alpha_v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(alpha_v), lane));
}

// the index of sample first + j as the counter word it is: the sum is formed in unsigned, so the lanes that draw past the last
// sample (their draws are never read) wrap instead of overflowing an int
__device__ __forceinline__ unsigned gs_sample(int first, int j) { return (unsigned)first + (unsigned)j; }

// cnt <= 4 consecutive floats from / to p: one 16-byte access (VEC; cnt == 4) or one element at a time; NT: streamed once
template <bool VEC, bool NT = false>
__device__ __forceinline__ void gs_get(const float* __restrict__ p, int cnt, float (&v)[4]) {
    if constexpr (VEC) {
        at_load<4, NT>(p, v);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float t[1] = {0.f};
            if (k < cnt) at_load<1, NT>(p + k, t);
            v[k] = t[0];
        }
    }
}
template <bool VEC>
__device__ __forceinline__ void gs_put(float* __restrict__ p, int cnt, const float (&v)[4]) {
    if constexpr (VEC) {
        at_store<4>(p, v);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) p[k] = v[k];
    }
}

// d[k] = x~[k] - b[k] for the group of elements from e (a multiple of 4) of sample s, b the group's elements of the drawn
// baseline; NOISE: sigma > 0
template <bool NOISE>
__device__ __forceinline__ void gs_difference(const float (&x)[4], const float (&b)[4], float sigma, long e, unsigned s,
                                              unsigned seed_lo, unsigned seed_hi, float (&d)[4]) {
    if constexpr (NOISE) {
        float z[4];
        ib_noise<4>(e, s, seed_lo, seed_hi, z);
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = fmaf(sigma, z[k], x[k]) - b[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = x[k] - b[k];
    }
}

// what the three entry points refuse alike
static int gs_check_draws(const char* what, int first, int n, int R) {
    SC_REQUIRE(R >= 1, "%s: bad arguments (R %d baselines: a bank holds at least 1)", what, R);
    SC_REQUIRE(n >= 0 && first >= 0, "%s: bad arguments (first %d, n %d: neither may be negative)", what, first, n);
    SC_REQUIRE((long)first + n <= 2147483647L, "%s: samples [%d, %ld) lie outside [0, 2^31 - 1]", what, first, (long)first + n);
    return SC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GS_THREADS) void gradshap_draws_kernel(int* __restrict__ picks, float* __restrict__ alphas,
                                                                    unsigned seed_lo, unsigned seed_hi, int first, int n, int R) {
    const int j = blockIdx.x * GS_THREADS + threadIdx.x;
    if (j >= n) return;
    int pick;
    float alpha;
    gs_draw(seed_lo, seed_hi, gs_sample(first, j), R, pick, alpha);
    if (picks) picks[j] = pick;
    if (alphas) alphas[j] = alpha;
}

extern "C" int scouter_gradshap_draws(int* picks, float* alphas, int seed_lo, int seed_hi, int first, int n, int R, void* stream) {
    if (int rc = gs_check_draws("gradshap_draws", first, n, R)) return rc;
    SC_REQUIRE((((uintptr_t)picks | (uintptr_t)alphas) & 3) == 0,
               "gradshap_draws: misaligned pointer (picks and alphas must be 4-byte aligned)");
    if (n == 0 || (!picks && !alphas)) return SC_OK;
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("gradshap_draws", st, 60.0 * n, 8.0 * n);
    hipLaunchKernelGGL(gradshap_draws_kernel, dim3((unsigned)sc_cdiv(n, GS_THREADS)), dim3(GS_THREADS), 0, st, picks, alphas,
                       (unsigned)seed_lo, (unsigned)seed_hi, first, n, R);
    return sc_check_launch("gradshap_draws");
}

// ---------------------------------------------------------------------------------------------------------------------------
template <bool VEC, bool NOISE>
__global__ __launch_bounds__(GS_THREADS) void gradshap_images_kernel(const float* __restrict__ image, const float* __restrict__ bank,
                                                                     float* __restrict__ out, float sigma, unsigned seed_lo,
                                                                     unsigned seed_hi, int first, int n, int R, long E) {
    const long e_own = 4 * ((long)blockIdx.x * GS_THREADS + threadIdx.x);    // the group of elements e .. e + 3
    const bool valid = e_own < E;
    const long e = valid ? e_own : 0;                          // (a thread past E stays for the lane reads and stores nothing)
    const int cnt = VEC ? 4 : (int)min(4L, E - e);
    const int j0 = blockIdx.y * GS_JT, rows = min(GS_JT, n - j0);
    float x[4], alpha[GS_JT], b[GS_JT][4];
    gs_get<VEC>(image + e, cnt, x);
    int pick_v;
    float alpha_v;                                             // lane l: the draw of row j0 + (l mod GS_JT)
    gs_draw(seed_lo, seed_hi, gs_sample(first, j0 + (int)(threadIdx.x & (GS_JT - 1))), R, pick_v, alpha_v);
#pragma unroll
    for (int u = 0; u < GS_JT; ++u) {                          // the drawn rows of the bank first, all in flight together
        if (u < rows) {                                        // (uniform over the workgroup, as is pick; 0 <= pick < R)
            const int pick = gs_lane_pick(pick_v, u);
            alpha[u] = gs_lane_alpha(alpha_v, u);
            gs_get<VEC>(bank + (long)pick * E + e, cnt, b[u]);
        }
    }                                                          // (the last lane read: per-thread branches may follow)
#pragma unroll
    for (int u = 0; u < GS_JT; ++u) {
        if (u < rows && valid) {
            float d[4], v[4];
            gs_difference<NOISE>(x, b[u], sigma, e, gs_sample(first, j0 + u), seed_lo, seed_hi, d);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = fmaf(alpha[u], d[k], b[u][k]);
            gs_put<VEC>(out + (long)(j0 + u) * E + e, cnt, v);
        }
    }
}

extern "C" int scouter_gradshap_images_f32(const float* image, const float* bank, float* out, float sigma, int seed_lo, int seed_hi,
                                           int first, int n, int R, long E, void* stream) {
    if (int rc = gs_check_draws("gradshap_images", first, n, R)) return rc;
    SC_REQUIRE(E >= 0, "gradshap_images: bad arguments (E %ld may not be negative)", E);
    SC_REQUIRE(sigma >= 0.f && sigma <= 3.0e38f, "gradshap_images: sigma = %g (it must be finite and not negative)", (double)sigma);
    const bool empty = n == 0 || E == 0;                       // (an empty tensor may have no storage: its pointer is not needed)
    SC_REQUIRE(empty || (image && bank && out), "gradshap_images: null pointer (image %p, bank %p, out %p)", (const void*)image,
               (const void*)bank, (void*)out);
    SC_REQUIRE((((uintptr_t)image | (uintptr_t)bank | (uintptr_t)out) & 3) == 0,
               "gradshap_images: misaligned pointer (image, bank and out must be 4-byte aligned)");
    if (empty) return SC_OK;
    SC_UNSUPPORTED((long)n * E < (1L << 31) && (double)R * (double)E < 2147483648.0,
                   "gradshap_images: a chunk of %d x %ld or a bank of %d x %ld elements is past the 32-bit offsets", n, E, R, E);
    SC_UNSUPPORTED(n <= 65535 * GS_JT, "gradshap_images: n = %d rows (at most %d per call)", n, 65535 * GS_JT);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = E % 4 == 0 && (((uintptr_t)image | (uintptr_t)bank | (uintptr_t)out) & 15) == 0;
    const dim3 grid((unsigned)sc_cdiv((E + 3) / 4, GS_THREADS), (unsigned)sc_cdiv(n, GS_JT));
    ScProfScope prof("gradshap_images", st, (sigma > 0.f ? 63.0 : 3.0) * n * (double)E, 4.0 * (2.0 * n + 1.0) * (double)E);
    auto kern = vec ? (sigma > 0.f ? gradshap_images_kernel<true, true> : gradshap_images_kernel<true, false>)
                    : (sigma > 0.f ? gradshap_images_kernel<false, true> : gradshap_images_kernel<false, false>);
    hipLaunchKernelGGL(kern, grid, dim3(GS_THREADS), 0, st, image, bank, out, sigma, (unsigned)seed_lo, (unsigned)seed_hi, first, n, R,
                       E);
    return sc_check_launch("gradshap_images");
}

// ---------------------------------------------------------------------------------------------------------------------------
// the terms of one sample onto the running sums of the group
template <bool NOISE>
__device__ __forceinline__ void gs_add_sample(const float (&g)[4], const float (&x)[4], const float (&b)[4], float sigma, long e,
                                              unsigned s, unsigned seed_lo, unsigned seed_hi, double inv_n, double (&a)[4]) {
    float d[4];
    gs_difference<NOISE>(x, b, sigma, e, s, seed_lo, seed_hi, d);
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = fma((double)g[k] * (double)d[k], inv_n, a[k]);
}

template <bool VEC, bool NOISE>
__global__ __launch_bounds__(GS_THREADS) void gradshap_accumulate_kernel(const float* __restrict__ grads,
                                                                         const float* __restrict__ image,
                                                                         const float* __restrict__ bank, double* __restrict__ acc,
                                                                         float sigma, double inv_n, unsigned seed_lo,
                                                                         unsigned seed_hi, int first, int n, int R, long E) {
    const long e_own = 4 * ((long)blockIdx.x * GS_THREADS + threadIdx.x);
    const bool valid = e_own < E;
    const long e = valid ? e_own : 0;                          // (a thread past E stays for the lane reads and stores nothing)
    const int cnt = VEC ? 4 : (int)min(4L, E - e);
    const int lane = threadIdx.x & 63;
    float x[4];
    double a[4];
    gs_get<VEC>(image + e, cnt, x);
    if constexpr (VEC) {
        at_load<4>(acc + e, a);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = k < cnt ? acc[e + k] : 0.0;
    }
    constexpr int U = GS_ROWS;
    for (int j0 = 0; j0 < n; j0 += 64) {                       // 64 samples per round: lane l draws for sample first + j0 + l
        const int m = min(64, n - j0);
        int pick_v;                                            // (the fraction is drawn with it and not needed here)
        float alpha_v;
        gs_draw(seed_lo, seed_hi, gs_sample(first, j0 + lane), R, pick_v, alpha_v);
        int t = 0;
        for (; t + U <= m; t += U) {                           // U gradient rows and their bank rows in flight; the additions
            const int j = j0 + t;                              // stay in j order
            float g[U][4], b[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int pick = gs_lane_pick(pick_v, t + u);    // (uniform over the wave; 0 <= pick < R)
                gs_get<VEC, true>(grads + (long)(j + u) * E + e, cnt, g[u]);
                gs_get<VEC>(bank + (long)pick * E + e, cnt, b[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                gs_add_sample<NOISE>(g[u], x, b[u], sigma, e, gs_sample(first, j + u), seed_lo, seed_hi, inv_n, a);
        }
        for (; t < m; ++t) {
            const int j = j0 + t;
            float g[4], b[4];
            const int pick = gs_lane_pick(pick_v, t);
            gs_get<VEC, true>(grads + (long)j * E + e, cnt, g);
            gs_get<VEC>(bank + (long)pick * E + e, cnt, b);
            gs_add_sample<NOISE>(g, x, b, sigma, e, gs_sample(first, j), seed_lo, seed_hi, inv_n, a);
        }
    }
    if (!valid) return;                                        // (after the last lane read)
    if constexpr (VEC) {
        at_store<4>(acc + e, a);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) acc[e + k] = a[k];
    }
}

extern "C" int scouter_gradshap_accumulate_f64(const float* grads, const float* image, const float* bank, double* acc, float sigma,
                                               double inv_n, int seed_lo, int seed_hi, int first, int n, int R, long E,
                                               void* stream) {
    if (int rc = gs_check_draws("gradshap_accumulate", first, n, R)) return rc;
    SC_REQUIRE(E >= 0, "gradshap_accumulate: bad arguments (E %ld may not be negative)", E);
    SC_REQUIRE(sigma >= 0.f && sigma <= 3.0e38f, "gradshap_accumulate: sigma = %g (it must be finite and not negative)",
               (double)sigma);
    SC_REQUIRE(inv_n - inv_n == 0.0, "gradshap_accumulate: inv_n = %g (it must be finite)", inv_n);
    const bool empty = n == 0 || E == 0;                       // (an empty tensor may have no storage: its pointer is not needed)
    SC_REQUIRE(empty || (grads && image && bank && acc), "gradshap_accumulate: null pointer (grads %p, image %p, bank %p, acc %p)",
               (const void*)grads, (const void*)image, (const void*)bank, (void*)acc);
    SC_REQUIRE((((uintptr_t)grads | (uintptr_t)image | (uintptr_t)bank) & 3) == 0 && ((uintptr_t)acc & 7) == 0,
               "gradshap_accumulate: misaligned pointer (grads, image and bank must be 4-byte, acc 8-byte aligned)");
    if (empty) return SC_OK;
    SC_UNSUPPORTED((long)n * E < (1L << 31) && (double)R * (double)E < 2147483648.0,
                   "gradshap_accumulate: a chunk of %d x %ld or a bank of %d x %ld elements is past the 32-bit offsets", n, E, R, E);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = E % 4 == 0 && (((uintptr_t)grads | (uintptr_t)image | (uintptr_t)bank | (uintptr_t)acc) & 15) == 0;
    const dim3 grid((unsigned)sc_cdiv((E + 3) / 4, GS_THREADS));
    ScProfScope prof("gradshap_accumulate", st, (sigma > 0.f ? 64.0 : 4.0) * n * (double)E, (8.0 * n + 4.0 + 16.0) * (double)E);
    auto kern = vec ? (sigma > 0.f ? gradshap_accumulate_kernel<true, true> : gradshap_accumulate_kernel<true, false>)
                    : (sigma > 0.f ? gradshap_accumulate_kernel<false, true> : gradshap_accumulate_kernel<false, false>);
    hipLaunchKernelGGL(kern, grid, dim3(GS_THREADS), 0, st, grads, image, bank, acc, sigma, inv_n, (unsigned)seed_lo, (unsigned)seed_hi,
                       first, n, R, E);
    return sc_check_launch("gradshap_accumulate");
}
