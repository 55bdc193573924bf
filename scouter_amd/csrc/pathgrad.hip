// Path and noise batches for the gradient methods that need many gradients per image (tools/attribution.py
// integrated_gradients / smoothgrad; the reference's captum_vis.py runs captum's IntegratedGradients and NoiseTunnel): the
// images of a chunk are written straight into one reused batch buffer, the model's own forward and backward produce the
// gradients, and the gradients are summed in fp64 in one fixed order.  Five streaming kernels, one thread per output element
// (or per four consecutive ones), no atomics, no partial sums except the optional grand total of attr_finish, which goes
// through two stages with a grid that depends on E alone -- two calls give the same bits.
//
// E = C H W is the flat element count of one image, e the flat index.
//
// path_images_kernel: out[j][e] = fmaf(alphas[first + j], image[e] - base[e], base[e]).  The fp32 difference is formed once per
//   element and serves the PG_JT values of j a thread owns (blockIdx.y tiles j).
// noise_images_kernel: out[j][e] = fmaf(sigma, z(seed, first + j, e), image[e]), z from Philox4x32-10 with the key
//   (seed_lo, seed_hi) and the counter (e / 4, first + j, 0, 0): the four output words serve the elements 4q .. 4q + 3 through
//   two Box-Muller pairs.  A thread owns one group q for its values of j, so an element's value depends on (seed, sample, e)
//   alone, not on the chunking and not on the vector / scalar path.
// grad_accumulate_kernel: acc[e] += sum_j w_j g[j][e] (and acc_sq[e] += sum_j w_j g[j][e]^2) in fp64, j ascending, starting
//   from the value in acc: the N terms split over calls at any point give the bits of one call.
// attr_finish_kernel: the fp32 result of a method from the fp64 sums (four modes), and, when asked for, sum_e (double)out[e].
// channel_mean_kernel: the mean over the channels in fp64, of the values or of their magnitudes.
//
// Every kernel has a 16-byte form (E, or H W, a multiple of 4 and every pointer 16-byte aligned) and a one-element form; the
// arithmetic of an element is one inlined expression shared by both, so they give the same bits.
#include "attr_common.h"

constexpr int PG_THREADS = 256;
constexpr int PG_JT = 8;                      // images of a chunk per thread (path / noise): the per-element work is shared
constexpr int PG_ROWS = 8;                    // gradient rows a thread of grad_accumulate has in flight
constexpr int PG_FIN_BLOCKS = 1024;           // at most this many partial sums of attr_finish's total (8 KB of workspace)

static inline bool pg_aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr,
                                const void* e = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & 15) == 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(PG_THREADS) void path_images_kernel(const float* __restrict__ image, const float* __restrict__ base,
                                                                 const float* __restrict__ alphas, float* __restrict__ out,
                                                                 int first, int n, long E) {
    constexpr int V = VEC ? 4 : 1;
    const long e = ((long)blockIdx.x * PG_THREADS + threadIdx.x) * V;
    if (e >= E) return;
    const int j0 = blockIdx.y * PG_JT, j1 = min(j0 + PG_JT, n);
    float b[V], d[V];
    if constexpr (VEC) {
        const f32x4 x = *(const f32x4*)(image + e);
        const f32x4 bb = base ? *(const f32x4*)(base + e) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) { b[k] = bb[k]; d[k] = x[k] - bb[k]; }
    } else {
        b[0] = base ? base[e] : 0.f;
        d[0] = image[e] - b[0];
    }
    for (int j = j0; j < j1; ++j) {
        const float a = alphas[first + j];                     // (uniform over the workgroup)
        float* __restrict__ o = out + (long)j * E + e;
        if constexpr (VEC) {
            f32x4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = fmaf(a, d[k], b[k]);
            *(f32x4*)o = v;
        } else {
            *o = fmaf(a, d[0], b[0]);
        }
    }
}

extern "C" int scouter_path_images_f32(const float* image, const float* base, const float* alphas, float* out, int first, int n,
                                       int N, long E, void* stream) {
    SC_REQUIRE(image && alphas && out, "path_images: null pointer (image %p, alphas %p, out %p)", (const void*)image,
               (const void*)alphas, (void*)out);
    SC_REQUIRE(n > 0 && N > 0 && E > 0, "path_images: bad arguments (n %d, N %d, E %ld: each must be at least 1)", n, N, E);
    SC_REQUIRE(first >= 0 && (long)first + n <= N, "path_images: steps [%d, %ld) lie outside [0, N = %d)", first, (long)first + n,
               N);
    SC_REQUIRE((((uintptr_t)image | (uintptr_t)base | (uintptr_t)alphas | (uintptr_t)out) & 3) == 0,
               "path_images: misaligned pointer (image, base, alphas and out must be 4-byte aligned)");
    SC_UNSUPPORTED((long)n * E < (1L << 31), "path_images: a chunk of %d x %ld elements is past the 32-bit offsets", n, E);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = E % 4 == 0 && pg_aligned16(image, base, out);
    const long items = vec ? E / 4 : E;
    const dim3 grid((unsigned)sc_cdiv(items, PG_THREADS), (unsigned)sc_cdiv(n, PG_JT));
    ScProfScope prof("path_images", st, (2.0 * n + 1.0) * (double)E, 4.0 * ((double)n * E + (base ? 2.0 : 1.0) * (double)E + n));
    if (vec)
        hipLaunchKernelGGL(path_images_kernel<true>, grid, dim3(PG_THREADS), 0, st, image, base, alphas, out, first, n, E);
    else
        hipLaunchKernelGGL(path_images_kernel<false>, grid, dim3(PG_THREADS), 0, st, image, base, alphas, out, first, n, E);
    return sc_check_launch("path_images");
}

// ---------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(PG_THREADS) void noise_images_kernel(const float* __restrict__ image, float* __restrict__ out,
                                                                  float sigma, unsigned seed_lo, unsigned seed_hi, int first,
                                                                  int n, long E) {
    const long q = (long)blockIdx.x * PG_THREADS + threadIdx.x;             // the group of elements 4q .. 4q + 3
    const long e = 4 * q;
    if (e >= E) return;
    const int cnt = VEC ? 4 : (int)min(4L, E - e);
    const int j0 = blockIdx.y * PG_JT, j1 = min(j0 + PG_JT, n);
    float x[4];
    if constexpr (VEC) {
        const f32x4 v = *(const f32x4*)(image + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = v[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = k < cnt ? image[e + k] : 0.f;
    }
    for (int j = j0; j < j1; ++j) {
        unsigned r[4];
        pg_philox((unsigned)q, (unsigned)(first + j), 0u, 0u, seed_lo, seed_hi, r);
        float z[4];
        pg_normal_pair(r[0], r[1], z[0], z[1]);
        pg_normal_pair(r[2], r[3], z[2], z[3]);
        float* __restrict__ o = out + (long)j * E + e;
        if constexpr (VEC) {
            f32x4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = fmaf(sigma, z[k], x[k]);
            *(f32x4*)o = v;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) o[k] = fmaf(sigma, z[k], x[k]);
        }
    }
}

extern "C" int scouter_noise_images_f32(const float* image, float* out, float sigma, int seed_lo, int seed_hi, int first, int n,
                                        long E, void* stream) {
    SC_REQUIRE(image && out, "noise_images: null pointer (image %p, out %p)", (const void*)image, (void*)out);
    SC_REQUIRE(n > 0 && E > 0, "noise_images: bad arguments (n %d, E %ld: each must be at least 1)", n, E);
    SC_REQUIRE(first >= 0 && (long)first + n < (1L << 31), "noise_images: samples [%d, %ld) lie outside [0, 2^31)", first,
               (long)first + n);
    SC_REQUIRE(sigma >= 0.f && sigma <= 3.0e38f, "noise_images: sigma = %g (it must be finite and not negative)", (double)sigma);
    SC_REQUIRE((((uintptr_t)image | (uintptr_t)out) & 3) == 0,
               "noise_images: misaligned pointer (image and out must be 4-byte aligned)");
    SC_UNSUPPORTED((long)n * E < (1L << 31), "noise_images: a chunk of %d x %ld elements is past the 32-bit offsets", n, E);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = E % 4 == 0 && pg_aligned16(image, out);
    const long groups = (E + 3) / 4;
    const dim3 grid((unsigned)sc_cdiv(groups, PG_THREADS), (unsigned)sc_cdiv(n, PG_JT));
    ScProfScope prof("noise_images", st, 60.0 * n * (double)E, 4.0 * ((double)n * E + (double)E));
    if (vec)
        hipLaunchKernelGGL(noise_images_kernel<true>, grid, dim3(PG_THREADS), 0, st, image, out, sigma, (unsigned)seed_lo,
                           (unsigned)seed_hi, first, n, E);
    else
        hipLaunchKernelGGL(noise_images_kernel<false>, grid, dim3(PG_THREADS), 0, st, image, out, sigma, (unsigned)seed_lo,
                           (unsigned)seed_hi, first, n, E);
    return sc_check_launch("noise_images");
}

// ---------------------------------------------------------------------------------------------------------------------------
// one term onto the running sums of an element: w g is exact in fp64 (24 + 24 bits), (w g) g takes one rounding inside the fma
__device__ __forceinline__ void pg_add_term(double w, float g, double& a, double& s, bool sq) {
    const double p = w * (double)g;
    a += p;
    if (sq) s = fma(p, (double)g, s);
}

template <int V>
__global__ __launch_bounds__(PG_THREADS) void grad_accumulate_kernel(const float* __restrict__ grads,
                                                                     const float* __restrict__ weights,
                                                                     double* __restrict__ acc, double* __restrict__ acc_sq,
                                                                     int first, int n, long E) {
    const long e = ((long)blockIdx.x * PG_THREADS + threadIdx.x) * V;
    if (e >= E) return;
    const bool sq = acc_sq != nullptr;                         // (uniform over the launch)
    double a[V], s[V];
    at_load<V>(acc + e, a);
    if (sq) {
        at_load<V>(acc_sq + e, s);
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) s[k] = 0.0;
    }
    const float* __restrict__ g = grads + e;
    int j = 0;
    constexpr int U = PG_ROWS;
    for (; j + U <= n; j += U) {                               // U rows in flight; the additions stay in j order
        float v[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) at_load<V, true>(g + (long)(j + u) * E, v[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double w = weights ? (double)weights[first + j + u] : 1.0;
#pragma unroll
            for (int k = 0; k < V; ++k) pg_add_term(w, v[u][k], a[k], s[k], sq);
        }
    }
    for (; j < n; ++j) {
        const double w = weights ? (double)weights[first + j] : 1.0;
        float v[V];
        at_load<V, true>(g + (long)j * E, v);
#pragma unroll
        for (int k = 0; k < V; ++k) pg_add_term(w, v[k], a[k], s[k], sq);
    }
    at_store<V>(acc + e, a);
    if (sq) at_store<V>(acc_sq + e, s);
}

extern "C" int scouter_grad_accumulate_f64(const float* grads, const float* weights, double* acc, double* acc_sq, int first,
                                           int n, int N, long E, void* stream) {
    SC_REQUIRE(grads && acc, "grad_accumulate: null pointer (grads %p, acc %p)", (const void*)grads, (void*)acc);
    SC_REQUIRE(n > 0 && N > 0 && E > 0, "grad_accumulate: bad arguments (n %d, N %d, E %ld: each must be at least 1)", n, N, E);
    SC_REQUIRE(first >= 0 && (long)first + n <= N, "grad_accumulate: terms [%d, %ld) lie outside [0, N = %d)", first,
               (long)first + n, N);
    SC_REQUIRE((((uintptr_t)grads | (uintptr_t)weights) & 3) == 0 && (((uintptr_t)acc | (uintptr_t)acc_sq) & 7) == 0,
               "grad_accumulate: misaligned pointer (grads and weights must be 4-byte, acc and acc_sq 8-byte aligned)");
    SC_REQUIRE(acc != acc_sq, "grad_accumulate: acc and acc_sq are the same buffer");
    SC_UNSUPPORTED((long)n * E < (1L << 31), "grad_accumulate: a chunk of %d x %ld elements is past the 32-bit offsets", n, E);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = E % 4 == 0 && pg_aligned16(grads, acc, acc_sq);
    const long items = vec ? E / 4 : E;
    const double sums = acc_sq ? 2.0 : 1.0;
    ScProfScope prof("grad_accumulate", st, 2.0 * sums * n * (double)E, 4.0 * n * (double)E + 16.0 * sums * (double)E);
    const dim3 grid((unsigned)sc_cdiv(items, PG_THREADS));
    if (vec)
        hipLaunchKernelGGL(grad_accumulate_kernel<4>, grid, dim3(PG_THREADS), 0, st, grads, weights, acc, acc_sq, first, n, E);
    else
        hipLaunchKernelGGL(grad_accumulate_kernel<1>, grid, dim3(PG_THREADS), 0, st, grads, weights, acc, acc_sq, first, n, E);
    return sc_check_launch("grad_accumulate");
}

// ---------------------------------------------------------------------------------------------------------------------------
// the result of element e by mode (include/scouter_hip.h SCOUTER_ATTR_*)
__device__ __forceinline__ float pg_finish(int mode, double a, double s, float x, float b, double inv_n) {
    switch (mode) {
        case 0: return (float)((double)(x - b) * a);
        case 1: return (float)(a * inv_n);
        case 2: return (float)(s * inv_n);
        default: {
            const double m = a * inv_n;
            return (float)fma(-m, m, s * inv_n);
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(PG_THREADS) void attr_finish_kernel(int mode, const double* __restrict__ acc,
                                                                 const double* __restrict__ acc_sq,
                                                                 const float* __restrict__ image, const float* __restrict__ base,
                                                                 double inv_n, float* __restrict__ out,
                                                                 double* __restrict__ partial, long E) {
    __shared__ double s_part[PG_THREADS / 64];
    constexpr int V = VEC ? 4 : 1;
    const long items = E / V;
    double sum = 0.0;
    for (long i = (long)blockIdx.x * PG_THREADS + threadIdx.x; i < items; i += (long)gridDim.x * PG_THREADS) {
        const long e = i * V;
        double a[V], s[V];
        float x[V], b[V], r[V];
#pragma unroll
        for (int k = 0; k < V; ++k) { a[k] = s[k] = 0.0; x[k] = b[k] = 0.f; }
        if constexpr (VEC) {
            if (mode != 2) {
                const f64x2 a0 = *(const f64x2*)(acc + e), a1 = *(const f64x2*)(acc + e + 2);
                a[0] = a0[0]; a[1] = a0[1]; a[2] = a1[0]; a[3] = a1[1];
            }
            if (mode >= 2) {
                const f64x2 s0 = *(const f64x2*)(acc_sq + e), s1 = *(const f64x2*)(acc_sq + e + 2);
                s[0] = s0[0]; s[1] = s0[1]; s[2] = s1[0]; s[3] = s1[1];
            }
            if (mode == 0) {
                const f32x4 xx = *(const f32x4*)(image + e);
                const f32x4 bb = base ? *(const f32x4*)(base + e) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < 4; ++k) { x[k] = xx[k]; b[k] = bb[k]; }
            }
        } else {
            if (mode != 2) a[0] = acc[e];
            if (mode >= 2) s[0] = acc_sq[e];
            if (mode == 0) { x[0] = image[e]; b[0] = base ? base[e] : 0.f; }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            r[k] = pg_finish(mode, a[k], s[k], x[k], b[k], inv_n);
            sum += (double)r[k];
        }
        if constexpr (VEC) *(f32x4*)(out + e) = f32x4{r[0], r[1], r[2], r[3]};
        else out[e] = r[0];
    }
    if (partial) {                                             // (uniform over the launch)
        const double t = at_block_sum<PG_THREADS / 64>(sum, s_part);
        if (threadIdx.x == 0) partial[blockIdx.x] = t;
    }
}

// total[0] = the partial sums of the first stage, added in a fixed order by one workgroup
__global__ __launch_bounds__(PG_THREADS) void attr_total_kernel(const double* __restrict__ partial, int count,
                                                                double* __restrict__ total) {
    __shared__ double s_part[PG_THREADS / 64];
    double v = 0.0;
    for (int i = threadIdx.x; i < count; i += PG_THREADS) v += partial[i];
    const double t = at_block_sum<PG_THREADS / 64>(v, s_part);
    if (threadIdx.x == 0) total[0] = t;
}

extern "C" size_t scouter_attr_finish_workspace_bytes(void) { return (size_t)PG_FIN_BLOCKS * sizeof(double); }

extern "C" int scouter_attr_finish_f32(int mode, const double* acc, const double* acc_sq, const float* image, const float* base,
                                       double inv_n, float* out, double* total, long E, void* ws, size_t ws_bytes, void* stream) {
    SC_REQUIRE(mode >= 0 && mode <= 3, "attr_finish: mode %d (0: integrated gradients, 1: mean, 2: mean of squares, 3: variance)",
               mode);
    SC_REQUIRE(out && (mode == 2 || acc) && (mode < 2 || acc_sq) && (mode != 0 || image),
               "attr_finish: null pointer (mode %d: acc %p, acc_sq %p, image %p, out %p)", mode, (const void*)acc,
               (const void*)acc_sq, (const void*)image, (void*)out);
    SC_REQUIRE(E > 0, "attr_finish: bad arguments (E %ld must be at least 1)", E);
    SC_REQUIRE((((uintptr_t)image | (uintptr_t)base | (uintptr_t)out) & 3) == 0 &&
                   (((uintptr_t)acc | (uintptr_t)acc_sq | (uintptr_t)total | (uintptr_t)ws) & 7) == 0,
               "attr_finish: misaligned pointer (image, base and out must be 4-byte, acc, acc_sq, total and ws 8-byte aligned)");
    SC_UNSUPPORTED(E < (1L << 31), "attr_finish: %ld elements are past the 32-bit offsets", E);
    if (total && (!ws || ws_bytes < scouter_attr_finish_workspace_bytes())) {
        sc_set_error("attr_finish: workspace too small (%zu < %zu bytes)", ws ? ws_bytes : (size_t)0,
                     scouter_attr_finish_workspace_bytes());
        return SC_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool vec = E % 4 == 0 && pg_aligned16(acc, acc_sq, image, base, out);
    const long items = vec ? E / 4 : E;
    long blocks = (items + PG_THREADS - 1) / PG_THREADS;       // (a function of E and the alignment alone: a fixed order)
    if (blocks > PG_FIN_BLOCKS) blocks = PG_FIN_BLOCKS;
    const double in_bytes = mode == 0 ? 8.0 + (base ? 8.0 : 4.0) : mode == 3 ? 16.0 : 8.0;
    ScProfScope prof("attr_finish", st, 4.0 * (double)E, (in_bytes + 4.0) * (double)E);
    double* partial = total ? (double*)ws : nullptr;
    if (vec)
        hipLaunchKernelGGL(attr_finish_kernel<true>, dim3((unsigned)blocks), dim3(PG_THREADS), 0, st, mode, acc, acc_sq, image,
                           base, inv_n, out, partial, E);
    else
        hipLaunchKernelGGL(attr_finish_kernel<false>, dim3((unsigned)blocks), dim3(PG_THREADS), 0, st, mode, acc, acc_sq, image,
                           base, inv_n, out, partial, E);
    if (total)
        hipLaunchKernelGGL(attr_total_kernel, dim3(1), dim3(PG_THREADS), 0, st, partial, (int)blocks, total);
    return sc_check_launch("attr_finish");
}

// ---------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(PG_THREADS) void channel_mean_kernel(const float* __restrict__ x, float* __restrict__ out, long M,
                                                                  int C, long HW, int absolute) {
    constexpr int V = VEC ? 4 : 1;
    const long per = HW / V;                                   // (VEC: H W is a multiple of 4)
    const long i = (long)blockIdx.x * PG_THREADS + threadIdx.x;
    if (i >= M * per) return;
    const long m = i / per, p = (i - m * per) * V;
    const float* __restrict__ src = x + m * C * HW + p;
    double s[V];
#pragma unroll
    for (int k = 0; k < V; ++k) s[k] = 0.0;
    for (int c = 0; c < C; ++c) {
        if constexpr (VEC) {
            const f32x4 v = __builtin_nontemporal_load((const f32x4*)(src + (long)c * HW));
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] += (double)(absolute ? fabsf(v[k]) : v[k]);
        } else {
            const float v = src[(long)c * HW];
            s[0] += (double)(absolute ? fabsf(v) : v);
        }
    }
    if constexpr (VEC) {
        f32x4 r;
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = (float)(s[k] / (double)C);
        *(f32x4*)(out + m * HW + p) = r;
    } else {
        out[m * HW + p] = (float)(s[0] / (double)C);
    }
}

extern "C" int scouter_channel_mean_f32(const float* x, float* out, long M, int C, long HW, int absolute, void* stream) {
    SC_REQUIRE(x && out, "channel_mean: null pointer (x %p, out %p)", (const void*)x, (void*)out);
    SC_REQUIRE(M > 0 && C > 0 && HW > 0, "channel_mean: bad arguments (M %ld, C %d, HW %ld: each must be at least 1)", M, C, HW);
    SC_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 3) == 0, "channel_mean: misaligned pointer (x and out must be 4-byte aligned)");
    SC_UNSUPPORTED(HW < (1L << 31) && M < (1L << 31) && (double)M * C * (double)HW < 2147483648.0,
                   "channel_mean: %ld x %d x %ld elements are past the 32-bit offsets", M, C, HW);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = HW % 4 == 0 && pg_aligned16(x, out);
    const long items = M * (vec ? HW / 4 : HW);
    ScProfScope prof("channel_mean", st, (double)M * C * (double)HW, 4.0 * (double)M * (C + 1.0) * (double)HW);
    const dim3 grid((unsigned)sc_cdiv(items, PG_THREADS));
    if (vec)
        hipLaunchKernelGGL(channel_mean_kernel<true>, grid, dim3(PG_THREADS), 0, st, x, out, M, C, HW, absolute);
    else
        hipLaunchKernelGGL(channel_mean_kernel<false>, grid, dim3(PG_THREADS), 0, st, x, out, M, C, HW, absolute);
    return sc_check_launch("channel_mean");
}
