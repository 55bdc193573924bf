// Grad-CAM++ (Chattopadhay et al., WACV 2018) and Smooth Grad-CAM++ (Omeiza et al. 2019) at the backbone's output, what the
// reference's torchcam_vis.py draws with torchcam's GradCAMpp / SmoothGradCAMpp (torchcam/cams/gradcam.py:104-272): the
// arithmetic between a feature gradient and a class map.  feat = A, NHWC [N = h w][C] fp32 per image, g = d log_prob / d A.
//
//   S[c] = sum_p g3[p][c] A[p][c]        den[p][c] = 2 g2[p][c] + S[c]        alpha[p][c] = g2[p][c] / den[p][c], 0 where den == 0
//   w[c] = sum_p alpha[p][c] max(gr[p][c], 0)                                  out[p] = sum_c w[c] A[p][c]   (relu: clamped at 0)
//
//   Grad-CAM++:        g2 = g^2 and g3 = g2 g in fp32, gr = g; S, den, alpha and w in fp32.
//   Smooth Grad-CAM++: g2 = acc2 / n and g3 = acc3 / n, the fp64 means of the squares and cubes of the n noisy samples' gradients
//                      (grad_powers_accumulate below), gr = the LAST sample's gradient, A the clean image's features; S, den,
//                      alpha and the sum of w in fp64, w rounded to fp32 once.
//
// gradcampp_kernel: ONE workgroup of 1024 threads per image, three passes, one template for both methods; the column sums and
//   the contraction are at_column_sums / at_contract_positions of attr_common.h, which gradcam_kernel runs too.
//   pass 1a: S[c].  The columns (float4 columns when C is a multiple of 4, single channels otherwise) are spread over the
//            threads, a wave reads 64 consecutive columns of one position; when there are fewer columns than threads the
//            positions are dealt to G = threads / columns groups, whose partial sums meet in LDS and are added in group order.
//   pass 1b: w[c], with the same column ownership: the thread that summed a column reads its S back from LDS.  The gradient
//            operand is read a second time (one image is N C 4 bytes, 0.66 MB at 9 x 9 x 2048: L2-sized).
//   pass 2:  out[p] = sum_c w[c] A[p][c], one wave per position: a lane takes every 64th column, the 64 partial sums meet in a
//            butterfly; out is written through a batch stride (a column of a [B][K][N] tensor).
//   LDS (dynamic): w fp32 [C] | S [C] | partial sums [4096] (only when there are fewer columns than threads), S and the
//   partial sums in the method's precision: at most 64 KiB (Grad-CAM++) / 96 KiB (smooth) at C = 8192.
//   One fixed summation order per output element and no atomics: two calls give the same bits.
//
// grad_powers_accumulate_kernel: acc2[e] += sum_j g[j][e]^2, acc3[e] += sum_j g[j][e]^3 in fp64, j ascending, starting from the
//   values in acc2 / acc3: g^2 is exact in fp64 (24 + 24 bits), g^2 g takes one rounding inside the fma that adds it.  A thread
//   owns an element (or four consecutive ones): the n terms split over calls at any point give the bits of one call.
#include <type_traits>

#include "attr_common.h"

constexpr int GP_ACC_THREADS = 256;

// SMOOTH false: gr = dfeat, acc2 / acc3 unused.  SMOOTH true: gr = the last sample's gradient, acc2 / acc3 the fp64 sums.
template <bool VEC, bool SMOOTH>
__global__ __launch_bounds__(AT_THREADS) void gradcampp_kernel(const float* __restrict__ feat, const float* __restrict__ gr,
                                                               const double* __restrict__ acc2, const double* __restrict__ acc3,
                                                               double n_samples, float* __restrict__ out, int N, int C,
                                                               long out_stride, int relu) {
    typedef typename std::conditional<SMOOTH, double, float>::type T;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    constexpr int V = VEC ? 4 : 1;
    float* __restrict__ s_w = (float*)s_raw;                                  // [C], padded to 16 bytes
    T* __restrict__ s_S = (T*)(s_raw + (size_t)((C + 3) / 4) * 16);          // [C]
    T* __restrict__ s_part = s_S + C;                                         // [AT_PART], when cols < AT_THREADS
    const long img = (long)blockIdx.x * N * C;
    const float* __restrict__ ft = feat + img;
    const float* __restrict__ gp = gr + img;

    const auto keep = [](T a) { return a; };                                  // (a column's total is stored as it is)

    // ---- pass 1a: S[c] = sum_p g3 A
    at_column_sums<V, T, T>(
        [&](int p, int q, const T (&)[V], T (&a)[V]) {
            const long e = (long)p * C + V * q;
            float A[V];
            at_load<V>(ft + e, A);
            if constexpr (SMOOTH) {
                double t[V];
                at_load<V>(acc3 + img + e, t);
#pragma unroll
                for (int k = 0; k < V; ++k) a[k] = fma(t[k] / n_samples, (double)A[k], a[k]);
            } else {
                float g[V];
                at_load<V>(gp + e, g);
#pragma unroll
                for (int k = 0; k < V; ++k) a[k] = fmaf(g[k] * g[k] * g[k], A[k], a[k]);
            }
        },
        keep, (const T*)nullptr, s_S, s_part, N, C);

    // ---- pass 1b: w[c] = sum_p alpha max(gr, 0), alpha = g2 / (2 g2 + S[c]) and 0 where the denominator is 0
    at_column_sums<V, T, float>(
        [&](int p, int q, const T (&S)[V], T (&a)[V]) {
            const long e = (long)p * C + V * q;
            float g[V];
            at_load<V>(gp + e, g);
            T g2[V];
            if constexpr (SMOOTH) {
                at_load<V>(acc2 + img + e, g2);
#pragma unroll
                for (int k = 0; k < V; ++k) g2[k] = g2[k] / n_samples;
            } else {
#pragma unroll
                for (int k = 0; k < V; ++k) g2[k] = g[k] * g[k];
            }
#pragma unroll
            for (int k = 0; k < V; ++k) {
                T den, alpha;
                if constexpr (SMOOTH) den = fma(2.0, g2[k], S[k]); else den = fmaf(2.f, g2[k], S[k]);
                alpha = den != (T)0 ? g2[k] / den : (T)0;
                if constexpr (SMOOTH) a[k] = fma(alpha, (double)fmaxf(g[k], 0.f), a[k]);
                else a[k] = fmaf(alpha, fmaxf(g[k], 0.f), a[k]);
            }
        },
        keep, (const T*)s_S, s_w, s_part, N, C);

    // ---- pass 2: one wave per position
    at_contract_positions<VEC>(ft, s_w, out + (long)blockIdx.x * out_stride, N, C, C / V, relu);
}

static size_t gp_lds_bytes(int C, size_t elem) {
    const int cols = C % 4 == 0 ? C / 4 : C;
    return (size_t)((C + 3) / 4) * 16 + ((size_t)C + (cols < AT_THREADS ? AT_PART : 0)) * elem;
}

extern "C" int scouter_gradcampp_f32(const float* feat, const float* dfeat, float* out, int B, int N, int C, long out_stride,
                                     int relu, void* stream) {
    SC_REQUIRE(feat && dfeat && out, "gradcampp: null pointer (feat %p, dfeat %p, out %p)", (const void*)feat,
               (const void*)dfeat, (void*)out);
    SC_REQUIRE(B > 0 && N > 0 && C > 0, "gradcampp: bad arguments (B %d, N %d, C %d: each must be at least 1)", B, N, C);
    SC_REQUIRE(((uintptr_t)feat & 15) == 0 && ((uintptr_t)dfeat & 15) == 0 && ((uintptr_t)out & 3) == 0,
               "gradcampp: misaligned pointer (feat and dfeat 16-byte, out 4-byte aligned)");
    SC_REQUIRE(out_stride >= N || B == 1, "gradcampp: output batch stride %ld is below N = %d", out_stride, N);
    SC_UNSUPPORTED(C <= AT_MAX_C, "gradcampp: C = %d channels (the channel weights live in LDS: at most %d)", C, AT_MAX_C);
    SC_UNSUPPORTED((long)N * C < (1L << 31), "gradcampp: image of %d x %d elements is past the 32-bit offsets", N, C);
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = gp_lds_bytes(C, sizeof(float));
    // per element: 4 flops for S, 7 for w, 2 for the map; feat and dfeat are each loaded twice (the second time from L2 at best)
    ScProfScope prof("gradcampp", st, 13.0 * B * (double)N * C, 4.0 * B * (4.0 * (double)N * C + N));
    if (C % 4 == 0) {
        sc_dyn_lds((const void*)gradcampp_kernel<true, false>, lds);
        hipLaunchKernelGGL((gradcampp_kernel<true, false>), dim3((unsigned)B), dim3(AT_THREADS), lds, st, feat, dfeat,
                           (const double*)nullptr, (const double*)nullptr, 1.0, out, N, C, out_stride, relu);
    } else {
        sc_dyn_lds((const void*)gradcampp_kernel<false, false>, lds);
        hipLaunchKernelGGL((gradcampp_kernel<false, false>), dim3((unsigned)B), dim3(AT_THREADS), lds, st, feat, dfeat,
                           (const double*)nullptr, (const double*)nullptr, 1.0, out, N, C, out_stride, relu);
    }
    return sc_check_launch("gradcampp");
}

extern "C" int scouter_gradcampp_smooth_f32(const float* feat, const double* acc2, const double* acc3, const float* glast,
                                            float* out, int n_samples, int B, int N, int C, long out_stride, int relu,
                                            void* stream) {
    SC_REQUIRE(feat && acc2 && acc3 && glast && out, "gradcampp_smooth: null pointer (feat %p, acc2 %p, acc3 %p, glast %p, out %p)",
               (const void*)feat, (const void*)acc2, (const void*)acc3, (const void*)glast, (void*)out);
    SC_REQUIRE(n_samples > 0 && B > 0 && N > 0 && C > 0,
               "gradcampp_smooth: bad arguments (n_samples %d, B %d, N %d, C %d: each must be at least 1)", n_samples, B, N, C);
    // (the 16-byte accesses exist only when C is a multiple of 4; a slice [k] of per-class sums with an odd image size is legal)
    const uintptr_t wide = C % 4 == 0 ? 15 : 0;
    SC_REQUIRE(((uintptr_t)feat & 15) == 0 && ((uintptr_t)glast & (wide | 3)) == 0 &&
                   (((uintptr_t)acc2 | (uintptr_t)acc3) & (wide | 7)) == 0 && ((uintptr_t)out & 3) == 0,
               "gradcampp_smooth: misaligned pointer (feat 16-byte, out 4-byte; acc2 / acc3 / glast 16-byte when C is a multiple "
               "of 4, else 8 / 8 / 4-byte aligned)");
    SC_REQUIRE(out_stride >= N || B == 1, "gradcampp_smooth: output batch stride %ld is below N = %d", out_stride, N);
    SC_UNSUPPORTED(C <= AT_MAX_C, "gradcampp_smooth: C = %d channels (the channel weights live in LDS: at most %d)", C, AT_MAX_C);
    SC_UNSUPPORTED((long)N * C < (1L << 31), "gradcampp_smooth: image of %d x %d elements is past the 32-bit offsets", N, C);
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = gp_lds_bytes(C, sizeof(double));
    // per element: 3 flops for S, 6 for w, 2 for the map; loads: acc3 + feat, acc2 + glast, feat = 28 bytes
    ScProfScope prof("gradcampp_smooth", st, 11.0 * B * (double)N * C, B * (28.0 * (double)N * C + 4.0 * N));
    if (C % 4 == 0) {
        sc_dyn_lds((const void*)gradcampp_kernel<true, true>, lds);
        hipLaunchKernelGGL((gradcampp_kernel<true, true>), dim3((unsigned)B), dim3(AT_THREADS), lds, st, feat, glast, acc2, acc3,
                           (double)n_samples, out, N, C, out_stride, relu);
    } else {
        sc_dyn_lds((const void*)gradcampp_kernel<false, true>, lds);
        hipLaunchKernelGGL((gradcampp_kernel<false, true>), dim3((unsigned)B), dim3(AT_THREADS), lds, st, feat, glast, acc2, acc3,
                           (double)n_samples, out, N, C, out_stride, relu);
    }
    return sc_check_launch("gradcampp_smooth");
}

// ---------------------------------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(GP_ACC_THREADS) void grad_powers_accumulate_kernel(const float* __restrict__ grads,
                                                                                double* __restrict__ acc2,
                                                                                double* __restrict__ acc3, int n, long E) {
    const long e = ((long)blockIdx.x * GP_ACC_THREADS + threadIdx.x) * V;
    if (e >= E) return;
    double a2[V], a3[V];
    at_load<V>(acc2 + e, a2);
    at_load<V>(acc3 + e, a3);
    for (int j = 0; j < n; ++j) {
        float g[V];
        at_load<V>(grads + (long)j * E + e, g);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const double d = (double)g[k], sq = d * d;         // (exact)
            a2[k] += sq;
            a3[k] = fma(sq, d, a3[k]);
        }
    }
    at_store<V>(acc2 + e, a2);
    at_store<V>(acc3 + e, a3);
}

extern "C" int scouter_grad_powers_accumulate(const float* grads, double* acc2, double* acc3, int n, long E, void* stream) {
    SC_REQUIRE(grads && acc2 && acc3, "grad_powers_accumulate: null pointer (grads %p, acc2 %p, acc3 %p)", (const void*)grads,
               (void*)acc2, (void*)acc3);
    SC_REQUIRE(n > 0 && E > 0, "grad_powers_accumulate: bad arguments (n %d, E %ld: each must be at least 1)", n, E);
    SC_REQUIRE(((uintptr_t)grads & 3) == 0 && (((uintptr_t)acc2 | (uintptr_t)acc3) & 7) == 0,
               "grad_powers_accumulate: misaligned pointer (grads must be 4-byte, acc2 and acc3 8-byte aligned)");
    SC_REQUIRE(acc2 != acc3, "grad_powers_accumulate: acc2 and acc3 are the same buffer");
    SC_UNSUPPORTED((long)n * E < (1L << 31), "grad_powers_accumulate: a chunk of %d x %ld elements is past the 32-bit offsets", n,
                   E);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = E % 4 == 0 && ((((uintptr_t)grads | (uintptr_t)acc2 | (uintptr_t)acc3) & 15) == 0);
    const long items = vec ? E / 4 : E;
    ScProfScope prof("grad_powers_accumulate", st, 4.0 * n * (double)E, 4.0 * n * (double)E + 32.0 * (double)E);
    const dim3 grid((unsigned)sc_cdiv(items, GP_ACC_THREADS));
    if (vec)
        hipLaunchKernelGGL(grad_powers_accumulate_kernel<4>, grid, dim3(GP_ACC_THREADS), 0, st, grads, acc2, acc3, n, E);
    else
        hipLaunchKernelGGL(grad_powers_accumulate_kernel<1>, grid, dim3(GP_ACC_THREADS), 0, st, grads, acc2, acc3, n, E);
    return sc_check_launch("grad_powers_accumulate");
}
