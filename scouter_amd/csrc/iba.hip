// Information-bottleneck attribution (Schulz, Sixt, Tombari, Landgraf, ICLR 2020; the reference's torchcam/IBA/pytorch.py, which
// torchcam_vis.py attaches to model.layer4): the mask side of one Adam step on the masks alpha [K][h][w][C] of one image's feature
// tensor x [h][w][C] (tools/attribution.py information_bottleneck), and the streaming estimator of the feature distribution.
// N = h w positions, E = N C neurons, rows j = k S + s.  One launch each, no atomics, every sum in one fixed order: two calls
// give the same bits, and a class's values do not depend on the other classes of the call.
//
// iba_sample_kernel / iba_step_kernel: a workgroup takes one class k and a tile of IB_TC channels at every position, V = 4
//   channels per thread through 16-byte accesses (C a multiple of 4, every pointer 16-byte aligned) or V = 1.  Four LDS arrays
//   [N][IB_TC]: sigmoid(alpha) and sigmoid(-alpha), then lambda = G(sigmoid(alpha)) and kappa = G(sigmoid(-alpha)), the window
//   (IbWindow, a kernel argument copied to LDS) applied over (h, w) through ib_reflect in (a, b) order by one fma per tap --
//   ib_fill_mask, the same code for both kernels.  kappa is formed from sigmoid(-alpha), not as 1 - lambda.
//   sample: z[j] = a ? fma(lambda, x, kappa e) : 0 with e = fma(max(std, min_std), eps[j], mean), clamped at 0 with relu; eps from
//     ib_noise under the counter (e / 4, first + j, 0, 0), generated, never stored.  cap = a ? -0.5 (1 + 2 ln kappa - (r lambda)^2
//     - kappa^2) : 0, r = (x - mean) / max(std, min_std), written when cap_out is given.  The samples of a class are dealt to the
//     threads in chunks of IB_SCH.
//   step: G_lambda = a ? sum_s dz[k S + s] (x - e_s) [z_s > 0 if relu] + (beta / E) (1 / kappa + r^2 lambda - kappa) : 0, the sum by
//     one fma per sample in ascending s, e_s and z_s from the expressions of sample (ib_sample_value); G_lambda replaces lambda
//     in LDS; G_alpha = sigmoid(alpha) sigmoid(-alpha) G^T(G_lambda), the adjoint as a gather over ib_sources; then Adam in place
//     (torch.optim.Adam's arithmetic, the bias corrections formed in fp64 on the host).  All positions of a channel live in one
//     workgroup, so every G_lambda of a channel exists before any alpha of it moves; alpha, adam_m and adam_v of a tile are read
//     and written by that workgroup alone.
// iba_estimate_kernel: one thread per neuron, Welford in fp64 over the rows of a batch in order -- count, mean, M2 -- and an int32
//   count of non-zero values; a batch split into chunks gives the same bits.
// iba_estimate_finish_kernel: mean, sqrt(M2 / (n - 1)) and nonzero / n > threshold as fp32.
// iba_bits_kernel: one thread per (k, position): sum_c cap in fp64 in ascending c, divided by ln 2.
#include "attr_common.h"

constexpr int IB_THREADS = 256;
constexpr int IB_TC = 32;                          // channels per workgroup: 128 bytes of every position's row
constexpr int IB_MAX_POS = 120;                    // positions h w: four LDS arrays of 120 x 32 floats = 60 KB, plus the window
constexpr int IB_SCH = 4;                          // samples per work item of iba_sample

struct IbFeat {
    const float* __restrict__ x;
    const float* __restrict__ mean;
    const float* __restrict__ std;
    const float* __restrict__ active;
    int h, w, C;
    float min_std;
};

// z of one neuron for one noise value, and e = the noise in feature units: ONE expression for iba_sample and iba_step
__device__ __forceinline__ float ib_sample_value(float lam, float kap, float x, float m, float sd, float eps, float& e) {
    e = fmaf(sd, eps, m);
    return fmaf(lam, x, kap * e);
}

// s_pos / s_neg / s_lam / s_kap [N][IB_TC] of class-k masks alpha_k and channels [c0, c0 + tc); ends in a barrier
template <int V>
__device__ __forceinline__ void ib_fill_mask(const float* __restrict__ alpha_k, const IbWindow& win, float* __restrict__ s_w,
                                             float* __restrict__ s_pos, float* __restrict__ s_neg, float* __restrict__ s_lam,
                                             float* __restrict__ s_kap, int h, int w, int C, int c0, int tc) {
    const int N = h * w, cols = tc / V, r = win.r, D = 2 * r + 1;
    for (int t = threadIdx.x; t < D * D; t += IB_THREADS) s_w[t] = win.w[t];
    for (int i = threadIdx.x; i < N * cols; i += IB_THREADS) {
        const int p = i / cols, q = i - p * cols;
        float a[V];
        at_load<V>(alpha_k + (long)p * C + c0 + V * q, a);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            s_pos[p * IB_TC + V * q + k] = 1.f / (1.f + expf(-a[k]));
            s_neg[p * IB_TC + V * q + k] = 1.f / (1.f + expf(a[k]));
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < N * cols; i += IB_THREADS) {
        const int p = i / cols, q = i - p * cols, y = p / w, x = p - y * w;
        float lam[V], kap[V];
#pragma unroll
        for (int k = 0; k < V; ++k) lam[k] = kap[k] = 0.f;
        for (int a = 0; a < D; ++a) {
            const int yy = ib_reflect(y + a - r, h);
            for (int b = 0; b < D; ++b) {
                const int src = (yy * w + ib_reflect(x + b - r, w)) * IB_TC + V * q;
                const float wt = s_w[a * D + b];
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    lam[k] = fmaf(wt, s_pos[src + k], lam[k]);
                    kap[k] = fmaf(wt, s_neg[src + k], kap[k]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            s_lam[p * IB_TC + V * q + k] = lam[k];
            s_kap[p * IB_TC + V * q + k] = kap[k];
        }
    }
    __syncthreads();
}

template <int V>
__device__ __forceinline__ void ib_store(float* __restrict__ p, const float (&v)[V]) {
    if constexpr (V == 4) *(f32x4*)p = f32x4{v[0], v[1], v[2], v[3]};
    else *p = v[0];
}

// ---------------------------------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(IB_THREADS) void iba_sample_kernel(IbFeat f, const float* __restrict__ alpha, float* __restrict__ z_out,
                                                                float* __restrict__ cap_out, IbWindow win, int S, unsigned seed_lo,
                                                                unsigned seed_hi, int first, int relu) {
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    __shared__ float s_w[IB_MAX_D * IB_MAX_D];
    const int N = f.h * f.w, C = f.C, k = blockIdx.y, c0 = blockIdx.x * IB_TC, tc = min(IB_TC, C - c0), cols = tc / V;
    const long E = (long)N * C;
    float *s_pos = s_mem, *s_neg = s_mem + N * IB_TC, *s_lam = s_mem + 2 * N * IB_TC, *s_kap = s_mem + 3 * N * IB_TC;
    ib_fill_mask<V>(alpha + (long)k * E, win, s_w, s_pos, s_neg, s_lam, s_kap, f.h, f.w, C, c0, tc);
    const int chunks = (S + IB_SCH - 1) / IB_SCH, per = N * cols;
    for (int i = threadIdx.x; i < chunks * per; i += IB_THREADS) {
        const int sc = i / per, rem = i - sc * per, p = rem / cols, q = rem - p * cols;
        const long e = (long)p * C + c0 + V * q;
        float x[V], m[V], sd[V], a[V];
        at_load<V>(f.x + e, x); at_load<V>(f.mean + e, m); at_load<V>(f.std + e, sd); at_load<V>(f.active + e, a);
        float lam[V], kap[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            sd[v] = fmaxf(sd[v], f.min_std);
            lam[v] = s_lam[p * IB_TC + V * q + v];
            kap[v] = s_kap[p * IB_TC + V * q + v];
        }
        if (sc == 0 && cap_out) {
            float cap[V];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float mu = (x[v] - m[v]) / sd[v] * lam[v];
                cap[v] = a[v] != 0.f ? -0.5f * (1.f + 2.f * logf(kap[v]) - mu * mu - kap[v] * kap[v]) : 0.f;
            }
            ib_store<V>(cap_out + (long)k * E + e, cap);
        }
        const int s1 = min(S, (sc + 1) * IB_SCH);
        for (int s = sc * IB_SCH; s < s1; ++s) {
            const int j = k * S + s;
            float eps[V], z[V];
            ib_noise<V>(e, (unsigned)(first + j), seed_lo, seed_hi, eps);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float en;
                const float zz = ib_sample_value(lam[v], kap[v], x[v], m[v], sd[v], eps[v], en);
                z[v] = a[v] != 0.f ? (relu ? fmaxf(zz, 0.f) : zz) : 0.f;
            }
            ib_store<V>(z_out + (long)j * E + e, z);
        }
    }
}

// the checks iba_sample and iba_step share; fills the window
static int ib_check(const char* what, int K, int S, int h, int w, int C, float sigma, float min_std, int first, int relu,
                    IbWindow& win) {
    SC_REQUIRE(K > 0 && S > 0 && h > 0 && w > 0 && C > 0, "%s: bad arguments (K %d, S %d, h %d, w %d, C %d: each must be at least 1)",
               what, K, S, h, w, C);
    SC_REQUIRE(sigma >= 0.f && sigma <= 3.0e38f, "%s: sigma = %g (positive and finite, or 0 for no smoothing)", what, (double)sigma);
    SC_REQUIRE(min_std > 0.f && min_std <= 3.0e38f, "%s: min_std = %g (it must be positive and finite)", what, (double)min_std);
    SC_REQUIRE(relu == 0 || relu == 1, "%s: relu = %d (0 or 1)", what, relu);
    SC_UNSUPPORTED(sigma <= 3.25f, "%s: sigma = %g needs a window radius above %d", what, (double)sigma, IB_MAX_R);
    const int r = ib_radius(sigma);
    SC_REQUIRE(r < h && r < w, "%s: a window of radius %d (sigma %g) needs h and w above it (h %d, w %d)", what, r, (double)sigma, h, w);
    SC_UNSUPPORTED((long)h * w <= IB_MAX_POS, "%s: %d x %d positions (at most %d)", what, h, w, IB_MAX_POS);
    SC_UNSUPPORTED(K <= 65535, "%s: K = %d classes (at most 65535 per call)", what, K);
    SC_UNSUPPORTED((double)K * S * h * w * C < 2147483648.0, "%s: %d x %d rows of %d x %d x %d elements are past the 32-bit offsets",
                   what, K, S, h, w, C);
    SC_REQUIRE(first >= 0 && (long)first + (long)K * S < (1L << 31), "%s: samples [%d, %ld) lie outside [0, 2^31)", what, first,
               (long)first + (long)K * S);
    ib_window(sigma, win);
    return SC_OK;
}

extern "C" int scouter_iba_sample_f32(const float* x, const float* mean, const float* std, const float* active, const float* alpha,
                                      float* z_out, float* cap_out, int K, int S, int h, int w, int C, float sigma, float min_std,
                                      int seed_lo, int seed_hi, int first, int relu, void* stream) {
    SC_REQUIRE(x && mean && std && active && alpha && z_out,
               "iba_sample: null pointer (x %p, mean %p, std %p, active %p, alpha %p, z_out %p)", (const void*)x, (const void*)mean,
               (const void*)std, (const void*)active, (const void*)alpha, (void*)z_out);
    IbWindow win;
    if (int rc = ib_check("iba_sample", K, S, h, w, C, sigma, min_std, first, relu, win)) return rc;
    const uintptr_t bits = (uintptr_t)x | (uintptr_t)mean | (uintptr_t)std | (uintptr_t)active | (uintptr_t)alpha | (uintptr_t)z_out |
                           (uintptr_t)cap_out;
    SC_REQUIRE((bits & 3) == 0, "iba_sample: misaligned pointer (every array must be 4-byte aligned)");
    hipStream_t st = (hipStream_t)stream;
    const IbFeat f{x, mean, std, active, h, w, C, min_std};
    const double E = (double)h * w * C;
    ScProfScope prof("iba_sample", st, 150.0 * K * S * E, 4.0 * E * ((double)K * S + K * (cap_out ? 6.0 : 5.0)));
    const dim3 grid((unsigned)sc_cdiv(C, IB_TC), (unsigned)K);
    const size_t lds = (size_t)4 * h * w * IB_TC * sizeof(float);
    if (C % 4 == 0 && (bits & 15) == 0)
        hipLaunchKernelGGL(iba_sample_kernel<4>, grid, dim3(IB_THREADS), lds, st, f, alpha, z_out, cap_out, win, S, (unsigned)seed_lo,
                           (unsigned)seed_hi, first, relu);
    else
        hipLaunchKernelGGL(iba_sample_kernel<1>, grid, dim3(IB_THREADS), lds, st, f, alpha, z_out, cap_out, win, S, (unsigned)seed_lo,
                           (unsigned)seed_hi, first, relu);
    return sc_check_launch("iba_sample");
}

// ---------------------------------------------------------------------------------------------------------------------------
struct IbAdam {
    float b1, omb1, b2, omb2, step, bc2_sqrt, eps;
};

template <int V>
__global__ __launch_bounds__(IB_THREADS) void iba_step_kernel(IbFeat f, float* __restrict__ alpha, const float* __restrict__ dz,
                                                              float* __restrict__ adam_m, float* __restrict__ adam_v, IbWindow win,
                                                              int S, unsigned seed_lo, unsigned seed_hi, int first, float beta_e,
                                                              IbAdam ad, int relu) {
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    __shared__ float s_w[IB_MAX_D * IB_MAX_D];
    const int N = f.h * f.w, C = f.C, k = blockIdx.y, c0 = blockIdx.x * IB_TC, tc = min(IB_TC, C - c0), cols = tc / V;
    const long E = (long)N * C;
    float *s_pos = s_mem, *s_neg = s_mem + N * IB_TC, *s_lam = s_mem + 2 * N * IB_TC, *s_kap = s_mem + 3 * N * IB_TC;
    ib_fill_mask<V>(alpha + (long)k * E, win, s_w, s_pos, s_neg, s_lam, s_kap, f.h, f.w, C, c0, tc);
    // G_lambda of every position of the tile, into s_lam: an item reads and writes its own slots only
    for (int i = threadIdx.x; i < N * cols; i += IB_THREADS) {
        const int p = i / cols, q = i - p * cols;
        const long e = (long)p * C + c0 + V * q;
        float x[V], m[V], sd[V], a[V], lam[V], kap[V], acc[V];
        at_load<V>(f.x + e, x); at_load<V>(f.mean + e, m); at_load<V>(f.std + e, sd); at_load<V>(f.active + e, a);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            sd[v] = fmaxf(sd[v], f.min_std);
            lam[v] = s_lam[p * IB_TC + V * q + v];
            kap[v] = s_kap[p * IB_TC + V * q + v];
            acc[v] = 0.f;
        }
        for (int s = 0; s < S; ++s) {
            const int j = k * S + s;
            float eps[V], g[V];
            ib_noise<V>(e, (unsigned)(first + j), seed_lo, seed_hi, eps);
            at_load<V, true>(dz + (long)j * E + e, g);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float en;
                const float zz = ib_sample_value(lam[v], kap[v], x[v], m[v], sd[v], eps[v], en);
                if (!relu || zz > 0.f) acc[v] = fmaf(g[v], x[v] - en, acc[v]);
            }
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float r = (x[v] - m[v]) / sd[v];
            const float gl = acc[v] + beta_e * (1.f / kap[v] + r * r * lam[v] - kap[v]);
            s_lam[p * IB_TC + V * q + v] = a[v] != 0.f ? gl : 0.f;
        }
    }
    __syncthreads();
    const int r = win.r, D = 2 * r + 1;
    for (int i = threadIdx.x; i < N * cols; i += IB_THREADS) {
        const int p = i / cols, q = i - p * cols, y = p / f.w, x = p - y * f.w;
        int uy[3], ux[3];
        const int ny = ib_sources(y, f.h, r, uy), nx = ib_sources(x, f.w, r, ux);
        float ga[V];
#pragma unroll
        for (int v = 0; v < V; ++v) ga[v] = 0.f;
        for (int iy = 0; iy < ny; ++iy)
            for (int ix = 0; ix < nx; ++ix)
                for (int a = 0; a < D; ++a) {
                    const int oy = uy[iy] - (a - r);                          // the output row whose tap a reads padded row uy
                    if (oy < 0 || oy >= f.h) continue;
                    for (int b = 0; b < D; ++b) {
                        const int ox = ux[ix] - (b - r);
                        if (ox < 0 || ox >= f.w) continue;
                        const float wt = s_w[a * D + b];
                        const int src = (oy * f.w + ox) * IB_TC + V * q;
#pragma unroll
                        for (int v = 0; v < V; ++v) ga[v] = fmaf(wt, s_lam[src + v], ga[v]);
                    }
                }
        const long e = (long)k * E + (long)p * C + c0 + V * q;
        float al[V], mm[V], vv[V];
        at_load<V>(alpha + e, al); at_load<V>(adam_m + e, mm); at_load<V>(adam_v + e, vv);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float g = s_pos[p * IB_TC + V * q + v] * s_neg[p * IB_TC + V * q + v] * ga[v];
            mm[v] = fmaf(ad.b1, mm[v], ad.omb1 * g);
            vv[v] = fmaf(ad.b2, vv[v], ad.omb2 * g * g);
            al[v] = al[v] - ad.step * (mm[v] / (sqrtf(vv[v]) / ad.bc2_sqrt + ad.eps));
        }
        ib_store<V>(alpha + e, al); ib_store<V>(adam_m + e, mm); ib_store<V>(adam_v + e, vv);
    }
}

extern "C" int scouter_iba_step_f32(const float* x, const float* mean, const float* std, const float* active, float* alpha,
                                    const float* dz, float* adam_m, float* adam_v, int K, int S, int h, int w, int C, float sigma,
                                    float min_std, int seed_lo, int seed_hi, int first, float beta, float lr, int t, int relu,
                                    void* stream) {
    SC_REQUIRE(x && mean && std && active && alpha && dz && adam_m && adam_v,
               "iba_step: null pointer (x %p, mean %p, std %p, active %p, alpha %p, dz %p, adam_m %p, adam_v %p)", (const void*)x,
               (const void*)mean, (const void*)std, (const void*)active, (void*)alpha, (const void*)dz, (void*)adam_m, (void*)adam_v);
    IbWindow win;
    if (int rc = ib_check("iba_step", K, S, h, w, C, sigma, min_std, first, relu, win)) return rc;
    SC_REQUIRE(beta >= 0.f && beta <= 3.0e38f && lr >= 0.f && lr <= 3.0e38f, "iba_step: beta = %g, lr = %g (finite and not negative)",
               (double)beta, (double)lr);
    SC_REQUIRE(t >= 0 && t < (1 << 24), "iba_step: t = %d (the iteration, 0 <= t < 2^24)", t);
    const uintptr_t bits = (uintptr_t)x | (uintptr_t)mean | (uintptr_t)std | (uintptr_t)active | (uintptr_t)alpha | (uintptr_t)dz |
                           (uintptr_t)adam_m | (uintptr_t)adam_v;
    SC_REQUIRE((bits & 3) == 0, "iba_step: misaligned pointer (every array must be 4-byte aligned)");
    hipStream_t st = (hipStream_t)stream;
    const IbFeat f{x, mean, std, active, h, w, C, min_std};
    const double E = (double)h * w * C;
    const double b1 = 0.9, b2 = 0.999;
    IbAdam ad;
    ad.b1 = (float)b1; ad.omb1 = (float)(1.0 - b1); ad.b2 = (float)b2; ad.omb2 = (float)(1.0 - b2);
    ad.step = (float)((double)lr / (1.0 - pow(b1, t + 1.0)));
    ad.bc2_sqrt = (float)sqrt(1.0 - pow(b2, t + 1.0));
    ad.eps = 1e-8f;
    ScProfScope prof("iba_step", st, 150.0 * K * S * E, 4.0 * E * ((double)K * S + K * 10.0));
    const dim3 grid((unsigned)sc_cdiv(C, IB_TC), (unsigned)K);
    const size_t lds = (size_t)4 * h * w * IB_TC * sizeof(float);
    const float beta_e = (float)((double)beta / E);
    if (C % 4 == 0 && (bits & 15) == 0)
        hipLaunchKernelGGL(iba_step_kernel<4>, grid, dim3(IB_THREADS), lds, st, f, alpha, dz, adam_m, adam_v, win, S, (unsigned)seed_lo,
                           (unsigned)seed_hi, first, beta_e, ad, relu);
    else
        hipLaunchKernelGGL(iba_step_kernel<1>, grid, dim3(IB_THREADS), lds, st, f, alpha, dz, adam_m, adam_v, win, S, (unsigned)seed_lo,
                           (unsigned)seed_hi, first, beta_e, ad, relu);
    return sc_check_launch("iba_step");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IB_THREADS) void iba_estimate_kernel(const float* __restrict__ feat, double* __restrict__ mean,
                                                                  double* __restrict__ m2, int* __restrict__ nonzero, long n0, int B,
                                                                  long E) {
    const long e = (long)blockIdx.x * IB_THREADS + threadIdx.x;
    if (e >= E) return;
    double mu = mean[e], s = m2[e];
    int nz = nonzero[e];
    for (int b = 0; b < B; ++b) {
        const double v = (double)feat[(long)b * E + e];
        const double d = v - mu;
        mu += d / (double)(n0 + b + 1);
        s = fma(d, v - mu, s);
        nz += v != 0.0 ? 1 : 0;
    }
    mean[e] = mu; m2[e] = s; nonzero[e] = nz;
}

extern "C" int scouter_iba_estimate_f64(const float* feat, double* mean, double* m2, int* nonzero, long n0, int B, long E,
                                        void* stream) {
    SC_REQUIRE(feat && mean && m2 && nonzero, "iba_estimate: null pointer (feat %p, mean %p, m2 %p, nonzero %p)", (const void*)feat,
               (void*)mean, (void*)m2, (void*)nonzero);
    SC_REQUIRE(B > 0 && E > 0 && n0 >= 0, "iba_estimate: bad arguments (B %d, E %ld: each at least 1; n0 %ld: not negative)", B, E, n0);
    SC_REQUIRE(n0 + B < (1L << 31), "iba_estimate: %ld samples are past the int32 non-zero count", n0 + B);
    SC_REQUIRE((((uintptr_t)feat | (uintptr_t)nonzero) & 3) == 0 && (((uintptr_t)mean | (uintptr_t)m2) & 7) == 0,
               "iba_estimate: misaligned pointer (feat and nonzero 4-byte, mean and m2 8-byte aligned)");
    SC_UNSUPPORTED((double)B * (double)E < 2147483648.0 * 1024.0 && E < (1L << 31) * (long)IB_THREADS,
                   "iba_estimate: %d rows of %ld elements are past the offsets", B, E);
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("iba_estimate", st, 6.0 * B * (double)E, (4.0 * B + 40.0) * (double)E);
    hipLaunchKernelGGL(iba_estimate_kernel, dim3((unsigned)sc_cdiv(E, IB_THREADS)), dim3(IB_THREADS), 0, st, feat, mean, m2, nonzero,
                       n0, B, E);
    return sc_check_launch("iba_estimate");
}

__global__ __launch_bounds__(IB_THREADS) void iba_estimate_finish_kernel(const double* __restrict__ mean, const double* __restrict__ m2,
                                                                         const int* __restrict__ nonzero, float* __restrict__ mean_out,
                                                                         float* __restrict__ std_out, float* __restrict__ active_out,
                                                                         long n, double threshold, long E) {
    const long e = (long)blockIdx.x * IB_THREADS + threadIdx.x;
    if (e >= E) return;
    mean_out[e] = (float)mean[e];
    std_out[e] = (float)sqrt(m2[e] / (double)(n - 1));
    active_out[e] = (double)nonzero[e] / (double)n > threshold ? 1.f : 0.f;
}

extern "C" int scouter_iba_estimate_finish_f32(const double* mean, const double* m2, const int* nonzero, float* mean_out,
                                               float* std_out, float* active_out, long n, double threshold, long E, void* stream) {
    SC_REQUIRE(mean && m2 && nonzero && mean_out && std_out && active_out,
               "iba_estimate_finish: null pointer (mean %p, m2 %p, nonzero %p, mean_out %p, std_out %p, active_out %p)",
               (const void*)mean, (const void*)m2, (const void*)nonzero, (void*)mean_out, (void*)std_out, (void*)active_out);
    SC_REQUIRE(n >= 2, "iba_estimate_finish: n = %ld samples (a standard deviation needs at least 2)", n);
    SC_REQUIRE(E > 0, "iba_estimate_finish: E = %ld (at least 1)", E);
    SC_REQUIRE(threshold == threshold, "iba_estimate_finish: threshold is NaN");
    SC_REQUIRE((((uintptr_t)nonzero | (uintptr_t)mean_out | (uintptr_t)std_out | (uintptr_t)active_out) & 3) == 0 &&
                   (((uintptr_t)mean | (uintptr_t)m2) & 7) == 0,
               "iba_estimate_finish: misaligned pointer (fp64 arrays 8-byte, the others 4-byte aligned)");
    SC_UNSUPPORTED(E < (1L << 31) * (long)IB_THREADS, "iba_estimate_finish: %ld elements are past the grid", E);
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("iba_estimate_finish", st, 4.0 * (double)E, 32.0 * (double)E);
    hipLaunchKernelGGL(iba_estimate_finish_kernel, dim3((unsigned)sc_cdiv(E, IB_THREADS)), dim3(IB_THREADS), 0, st, mean, m2, nonzero,
                       mean_out, std_out, active_out, n, threshold, E);
    return sc_check_launch("iba_estimate_finish");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IB_THREADS) void iba_bits_kernel(const float* __restrict__ cap, float* __restrict__ out, long rows, int C) {
    const long i = (long)blockIdx.x * IB_THREADS + threadIdx.x;
    if (i >= rows) return;
    const float* __restrict__ row = cap + i * C;
    double a = 0.0;
    for (int c = 0; c < C; ++c) a += (double)row[c];
    out[i] = (float)(a / 0.6931471805599453);
}

extern "C" int scouter_iba_bits_f32(const float* cap, float* out, long rows, int C, void* stream) {
    SC_REQUIRE(cap && out, "iba_bits: null pointer (cap %p, out %p)", (const void*)cap, (void*)out);
    SC_REQUIRE(rows > 0 && C > 0, "iba_bits: bad arguments (rows %ld, C %d: each must be at least 1)", rows, C);
    SC_REQUIRE((((uintptr_t)cap | (uintptr_t)out) & 3) == 0, "iba_bits: misaligned pointer (cap and out must be 4-byte aligned)");
    SC_UNSUPPORTED((double)rows * C < 2147483648.0, "iba_bits: %ld rows of %d channels are past the 32-bit offsets", rows, C);
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("iba_bits", st, (double)rows * C, 4.0 * ((double)rows * C + (double)rows));
    hipLaunchKernelGGL(iba_bits_kernel, dim3((unsigned)sc_cdiv(rows, IB_THREADS)), dim3(IB_THREADS), 0, st, cap, out, rows, C);
    return sc_check_launch("iba_bits");
}
