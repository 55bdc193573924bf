// Infidelity and max-sensitivity of an explanation (Yeh et al., NeurIPS 2019, "On the (In)fidelity and Sensitivity of
// Explanations"; captum's infidelity and sensitivity_max, the last two columns of the SCOUTER paper's comparison): everything
// around the model's forwards and the explanation method's calls (tools/attribution.py infidelity / sensitivity_max).  One image
// x of E = C H W elements (e the flat index, HW = H W), a stream of N perturbed copies of it that goes through the model (or the
// explanation method) in chunks [first, first + n), and per-sample fp64 arrays [K][N] that the chunks fill.  Every kernel has one
// fixed order per output element and no atomics, and the value of an output element does not depend on the chunking.
//
// perturb_dots_kernel: dots[k][first + j] = sum_e a_k[e] I_j[e] with I_j[e] = -sigma z(seed, first + j, e), z the standard normal
//   of noise_images (attr_common.h pg_philox / pg_normal_pair, the counter (e / 4, first + j, 0, 0)), regenerated and never read
//   from a buffer.  a_k is FULL, [E], or a MAP, [HW], that counts for every channel: a_k[e] = m_k[e mod HW].  A thread owns the
//   groups q = 4q .. 4q + 3 it strides over, in ascending q; per group it loads the FD_KT attributions of its class tile
//   (blockIdx.z) once, then per sample of its sample tile (blockIdx.y, FD_JT samples) generates the four z, forms
//   p = -(double)sigma * (double)z (exact) and adds acc[k][j] = fma((double)a_k[e], p, acc[k][j]) for e = 4q .. 4q + 3 in that
//   order.  Then: a butterfly over the wave, the four waves added in order through LDS, one partial sum per workgroup into the
//   workspace.  perturb_dots_total_kernel adds the workgroups' partial sums in ascending workgroup order, starting from 0 (one
//   wave per sum: 64 partial sums are loaded at a time, one per lane, and added lane by lane).  The grid's x extent is
//   a function of E alone (min(ceil(ceil(E / 4) / 256), FD_MAX_BLOCKS)), and a sample's sums involve no other sample: the same
//   bits for any chunking.  The 16-byte form (the attributions' own length a multiple of 4 and a 16-byte aligned pointer) and
//   the one-element form differ in the loads alone.
// uniform_images_kernel: out[j][e] = fmaf(radius, d(seed, first + j, e), image[e]), d = fmaf(2, pg_uniform(word), -1) (exact:
//   ((2 (r >> 9) + 1) - 2^23) 2^-23, never 0, inside (-1, 1)), the words from Philox with the counter (e / 4, first + j, 1, 0):
//   the twin of noise_images_kernel on a stream of its own.
// output_deltas_kernel: delta[k][first + j] = F((double)out[0][c_k]) - F((double)out[1 + j][c_k]), F the identity or exp; one
//   thread per (k, j).
// map_distances_kernel: one workgroup per (j, k); a thread adds (A_j[m] - A_0[m])^2 (the difference formed in fp64) and
//   A_0[m]^2, each by one fma, for m = tid, tid + 256, ... in ascending m, then the butterfly and the waves in order;
//   term = sqrt(num / den), den replaced by 1 when it is 0.  den is recomputed by every workgroup from row 0 of the same call, in
//   the same order: the same bits for every j.
// infidelity_finish_kernel / sensitivity_finish_kernel: one thread per row, the N samples in ascending j.
#include "attr_common.h"

constexpr int FD_THREADS = 256, FD_WAVES = FD_THREADS / 64;
constexpr int FD_KT = 4;                      // attributions per thread (perturb_dots): one z serves them all
constexpr int FD_JT = 4;                      // samples per thread (perturb_dots): one load of the attributions serves them all
constexpr int FD_MAX_BLOCKS = 256;            // workgroups along the elements (perturb_dots); the threads stride over the rest
constexpr int FD_IMG_JT = 8;                  // images of a chunk per thread (uniform_images), as in noise_images

static inline int fd_dot_blocks(long E) {
    const long b = ((E + 3) / 4 + FD_THREADS - 1) / FD_THREADS;
    return (int)(b > FD_MAX_BLOCKS ? FD_MAX_BLOCKS : b);
}

// the chunk [first, first + n) of a stream of N samples
static int fd_check_chunk(const char* what, int first, int n, int N) {
    SC_REQUIRE(n > 0 && N > 0, "%s: bad arguments (n %d, N %d: each must be at least 1)", what, n, N);
    SC_REQUIRE(first >= 0 && (long)first + n <= N, "%s: samples [%d, %ld) lie outside [0, N = %d)", what, first, (long)first + n, N);
    return SC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(FD_THREADS) void perturb_dots_kernel(const float* __restrict__ attrs, double* __restrict__ partial,
                                                                  float sigma, unsigned seed_lo, unsigned seed_hi, int first,
                                                                  int n, int K, unsigned E, unsigned A) {
    __shared__ double s_part[FD_WAVES][FD_KT * FD_JT];
    const int tid = threadIdx.x;
    const int j0 = blockIdx.y * FD_JT, nj = min(FD_JT, n - j0);               // (uniform over the workgroup)
    const int k0 = blockIdx.z * FD_KT, nk = min(FD_KT, K - k0);
    const unsigned groups = (E + 3u) / 4u;
    const double minus_sigma = -(double)sigma;
    double acc[FD_KT][FD_JT];
#pragma unroll
    for (int k = 0; k < FD_KT; ++k)
#pragma unroll
        for (int j = 0; j < FD_JT; ++j) acc[k][j] = 0.0;
    for (unsigned q = blockIdx.x * FD_THREADS + tid; q < groups; q += gridDim.x * FD_THREADS) {
        const unsigned e = 4u * q;
        const int cnt = VEC ? 4 : (int)min(4u, E - e);
        float a[FD_KT][4];
#pragma unroll
        for (int k = 0; k < FD_KT; ++k) {
            if (k < nk) {
                const float* __restrict__ src = attrs + (long)(k0 + k) * A;
                if constexpr (VEC) {
                    at_load<4>(src + e % A, a[k]);                            // (A a multiple of 4: the four stay inside one plane)
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) a[k][i] = i < cnt ? src[(e + i) % A] : 0.f;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) a[k][i] = 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < FD_JT; ++j) {
            if (j < nj) {
                unsigned r[4];
                pg_philox(q, (unsigned)(first + j0 + j), 0u, 0u, seed_lo, seed_hi, r);
                float z[4];
                pg_normal_pair(r[0], r[1], z[0], z[1]);
                pg_normal_pair(r[2], r[3], z[2], z[3]);
                double p[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) p[i] = minus_sigma * (double)z[i];             // exact: 24 x 24 bits
#pragma unroll
                for (int k = 0; k < FD_KT; ++k)
                    if (k < nk) {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (i < cnt) acc[k][j] = fma((double)a[k][i], p[i], acc[k][j]);
                    }
            }
        }
    }
    const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int k = 0; k < FD_KT; ++k)
#pragma unroll
        for (int j = 0; j < FD_JT; ++j) {
            if (k < nk) {                                                     // (uniform over the workgroup)
                const double v = wave_sum_d(acc[k][j]);
                if (lane == 0) s_part[wv][k * FD_JT + j] = v;
            }
        }
    __syncthreads();
    if (tid < FD_KT * FD_JT) {
        const int k = tid / FD_JT, j = tid - k * FD_JT;
        if (k < nk && j < nj) {
            double t = s_part[0][tid];
#pragma unroll
            for (int w = 1; w < FD_WAVES; ++w) t += s_part[w][tid];
            partial[((long)(k0 + k) * n + j0 + j) * gridDim.x + blockIdx.x] = t;
        }
    }
}

// lane l's value of v in every lane (l uniform over the wave)
__device__ __forceinline__ double fd_read_lane(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// dots[k][first + j] = the workgroups' partial sums [K][n][blocks] of the first stage, added in workgroup order starting from 0:
// one wave per sum loads 64 partial sums at a time, one per lane, and adds them lane by lane
__global__ __launch_bounds__(FD_THREADS) void perturb_dots_total_kernel(const double* __restrict__ partial,
                                                                        double* __restrict__ dots, int blocks, int first, int n,
                                                                        int N, int K) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * FD_WAVES + (threadIdx.x >> 6);       // (uniform over the wave)
    if (i >= (long)K * n) return;
    const double* __restrict__ p = partial + i * blocks;
    double t = 0.0;
    for (int b0 = 0; b0 < blocks; b0 += 64) {
        const double v = b0 + lane < blocks ? p[b0 + lane] : 0.0;
        const int cnt = min(64, blocks - b0);
        for (int l = 0; l < cnt; ++l) t += fd_read_lane(v, l);
    }
    const int k = (int)(i / n), j = (int)(i - (long)k * n);
    if (lane == 0) dots[(long)k * N + first + j] = t;
}

extern "C" size_t scouter_perturb_dots_workspace_bytes(int n, int K, long E) {
    if (n < 1 || K < 1 || E < 1) return 0;
    return (size_t)fd_dot_blocks(E) * (size_t)K * (size_t)n * sizeof(double);
}

extern "C" int scouter_perturb_dots_f64(const float* attrs, double* dots, float sigma, int seed_lo, int seed_hi, int first, int n,
                                        int N, int K, long E, long A, void* ws, size_t ws_bytes, void* stream) {
    SC_REQUIRE(attrs && dots && ws, "perturb_dots: null pointer (attrs %p, dots %p, ws %p)", (const void*)attrs, (void*)dots, ws);
    SC_REQUIRE(K > 0 && E > 0 && A > 0, "perturb_dots: bad arguments (K %d, E %ld, A %ld: each must be at least 1)", K, E, A);
    if (int rc = fd_check_chunk("perturb_dots", first, n, N)) return rc;
    SC_REQUIRE(A <= E && E % A == 0, "perturb_dots: attributions of %ld elements for an image of %ld (E itself, or H W dividing it)",
               A, E);
    SC_REQUIRE(sigma >= 0.f && sigma <= 3.0e38f, "perturb_dots: sigma = %g (it must be finite and not negative)", (double)sigma);
    SC_REQUIRE(((uintptr_t)attrs & 3) == 0 && (((uintptr_t)dots | (uintptr_t)ws) & 7) == 0,
               "perturb_dots: misaligned pointer (attrs must be 4-byte, dots and ws 8-byte aligned)");
    SC_UNSUPPORTED(E < (1L << 31) && (long)K * A < (1L << 31),
                   "perturb_dots: an image of %ld elements or %d attributions of %ld are past the 32-bit offsets", E, K, A);
    SC_UNSUPPORTED(n <= 65535 * FD_JT && K <= 65535 * FD_KT, "perturb_dots: n = %d samples, K = %d attributions (at most %d and %d "
                   "per call)", n, K, 65535 * FD_JT, 65535 * FD_KT);
    if (ws_bytes < scouter_perturb_dots_workspace_bytes(n, K, E)) {
        sc_set_error("perturb_dots: workspace too small (%zu < %zu bytes)", ws_bytes, scouter_perturb_dots_workspace_bytes(n, K, E));
        return SC_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool vec = A % 4 == 0 && ((uintptr_t)attrs & 15) == 0;
    const int blocks = fd_dot_blocks(E);
    const dim3 grid((unsigned)blocks, (unsigned)sc_cdiv(n, FD_JT), (unsigned)sc_cdiv(K, FD_KT));
    double* partial = (double*)ws;
    {
        ScProfScope prof("perturb_dots", st, (60.0 * sc_cdiv(K, FD_KT) + 2.0 * K) * n * (double)E,
                         4.0 * K * (double)E * sc_cdiv(n, FD_JT) + 8.0 * blocks * (double)K * n);
        if (vec)
            hipLaunchKernelGGL(perturb_dots_kernel<true>, grid, dim3(FD_THREADS), 0, st, attrs, partial, sigma, (unsigned)seed_lo,
                               (unsigned)seed_hi, first, n, K, (unsigned)E, (unsigned)A);
        else
            hipLaunchKernelGGL(perturb_dots_kernel<false>, grid, dim3(FD_THREADS), 0, st, attrs, partial, sigma, (unsigned)seed_lo,
                               (unsigned)seed_hi, first, n, K, (unsigned)E, (unsigned)A);
    }
    if (int rc = sc_check_launch("perturb_dots")) return rc;
    {
        ScProfScope prof("perturb_dots_total", st, (double)blocks * K * n, 8.0 * (blocks + 1.0) * (double)K * n);
        hipLaunchKernelGGL(perturb_dots_total_kernel, dim3((unsigned)sc_cdiv((long)K * n, FD_WAVES)), dim3(FD_THREADS), 0, st,
                           partial, dots, blocks, first, n, N, K);
    }
    return sc_check_launch("perturb_dots");
}

// ---------------------------------------------------------------------------------------------------------------------------
// a random word -> 2 u - 1 = ((2 (r >> 9) + 1) - 2^23) 2^-23: an odd multiple of 2^-23 below 1 in magnitude, so the fma is exact
__device__ __forceinline__ float fd_signed_uniform(unsigned r) { return fmaf(2.f, pg_uniform(r), -1.f); }

template <bool VEC>
__global__ __launch_bounds__(FD_THREADS) void uniform_images_kernel(const float* __restrict__ image, float* __restrict__ out,
                                                                    float radius, unsigned seed_lo, unsigned seed_hi, int first,
                                                                    int n, long E) {
    const long q = (long)blockIdx.x * FD_THREADS + threadIdx.x;             // the group of elements 4q .. 4q + 3
    const long e = 4 * q;
    if (e >= E) return;
    const int cnt = VEC ? 4 : (int)min(4L, E - e);
    const int j0 = blockIdx.y * FD_IMG_JT, j1 = min(j0 + FD_IMG_JT, n);
    float x[4];
    if constexpr (VEC) {
        at_load<4>(image + e, x);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = k < cnt ? image[e + k] : 0.f;
    }
    for (int j = j0; j < j1; ++j) {
        unsigned r[4];
        pg_philox((unsigned)q, (unsigned)(first + j), 1u, 0u, seed_lo, seed_hi, r);
        float* __restrict__ o = out + (long)j * E + e;
        if constexpr (VEC) {
            f32x4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = fmaf(radius, fd_signed_uniform(r[k]), x[k]);
            *(f32x4*)o = v;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) o[k] = fmaf(radius, fd_signed_uniform(r[k]), x[k]);
        }
    }
}

extern "C" int scouter_uniform_images_f32(const float* image, float* out, float radius, int seed_lo, int seed_hi, int first, int n,
                                          long E, void* stream) {
    SC_REQUIRE(image && out, "uniform_images: null pointer (image %p, out %p)", (const void*)image, (void*)out);
    SC_REQUIRE(n > 0 && E > 0, "uniform_images: bad arguments (n %d, E %ld: each must be at least 1)", n, E);
    SC_REQUIRE(first >= 0 && (long)first + n < (1L << 31), "uniform_images: samples [%d, %ld) lie outside [0, 2^31)", first,
               (long)first + n);
    SC_REQUIRE(radius >= 0.f && radius <= 3.0e38f, "uniform_images: radius = %g (it must be finite and not negative)",
               (double)radius);
    SC_REQUIRE((((uintptr_t)image | (uintptr_t)out) & 3) == 0,
               "uniform_images: misaligned pointer (image and out must be 4-byte aligned)");
    SC_UNSUPPORTED((long)n * E < (1L << 31), "uniform_images: a chunk of %d x %ld elements is past the 32-bit offsets", n, E);
    SC_UNSUPPORTED(n <= 65535 * FD_IMG_JT, "uniform_images: n = %d samples (at most %d per call)", n, 65535 * FD_IMG_JT);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = E % 4 == 0 && ((((uintptr_t)image | (uintptr_t)out) & 15) == 0);
    const long groups = (E + 3) / 4;
    const dim3 grid((unsigned)sc_cdiv(groups, FD_THREADS), (unsigned)sc_cdiv(n, FD_IMG_JT));
    ScProfScope prof("uniform_images", st, 20.0 * n * (double)E, 4.0 * ((double)n * E + (double)E));
    if (vec)
        hipLaunchKernelGGL(uniform_images_kernel<true>, grid, dim3(FD_THREADS), 0, st, image, out, radius, (unsigned)seed_lo,
                           (unsigned)seed_hi, first, n, E);
    else
        hipLaunchKernelGGL(uniform_images_kernel<false>, grid, dim3(FD_THREADS), 0, st, image, out, radius, (unsigned)seed_lo,
                           (unsigned)seed_hi, first, n, E);
    return sc_check_launch("uniform_images");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FD_THREADS) void output_deltas_kernel(const float* __restrict__ out, const int* __restrict__ cols,
                                                                   double* __restrict__ deltas, int first, int n, int N, int K,
                                                                   int n_classes, int of) {
    const long i = (long)blockIdx.x * FD_THREADS + threadIdx.x;
    if (i >= (long)K * n) return;
    const int k = (int)(i / n), j = (int)(i - (long)k * n);
    const int c = min(max(cols[k], 0), n_classes - 1);                        // (the host refuses an index outside)
    double clean = (double)out[c], moved = (double)out[(long)(1 + j) * n_classes + c];
    if (of == 1) { clean = exp(clean); moved = exp(moved); }
    deltas[(long)k * N + first + j] = clean - moved;
}

extern "C" int scouter_output_deltas_f64(const float* out, const int* cols, double* deltas, int first, int n, int N, int K,
                                         int n_classes, int of, void* stream) {
    SC_REQUIRE(out && cols && deltas, "output_deltas: null pointer (out %p, cols %p, deltas %p)", (const void*)out,
               (const void*)cols, (void*)deltas);
    SC_REQUIRE(K > 0 && n_classes > 0, "output_deltas: bad arguments (K %d, n_classes %d: each must be at least 1)", K, n_classes);
    if (int rc = fd_check_chunk("output_deltas", first, n, N)) return rc;
    SC_REQUIRE(of == 0 || of == 1, "output_deltas: of = %d (0: the log-probability, 1: the probability)", of);
    SC_REQUIRE((((uintptr_t)out | (uintptr_t)cols) & 3) == 0 && ((uintptr_t)deltas & 7) == 0,
               "output_deltas: misaligned pointer (out and cols must be 4-byte, deltas 8-byte aligned)");
    SC_UNSUPPORTED((1L + n) * n_classes < (1L << 31) && (long)K * n <= 65535L * FD_THREADS,
                   "output_deltas: %d rows of %d outputs for %d classes are past the 32-bit offsets", 1 + n, n_classes, K);
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("output_deltas", st, (double)K * n, 20.0 * K * n);
    hipLaunchKernelGGL(output_deltas_kernel, dim3((unsigned)sc_cdiv((long)K * n, FD_THREADS)), dim3(FD_THREADS), 0, st, out, cols,
                       deltas, first, n, N, K, n_classes, of);
    return sc_check_launch("output_deltas");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FD_THREADS) void map_distances_kernel(const float* __restrict__ maps, double* __restrict__ terms,
                                                                   int first, int N, int K, long M) {
    __shared__ double s_num[FD_WAVES], s_den[FD_WAVES];
    const int j = blockIdx.x, k = blockIdx.y;
    const float* __restrict__ a0 = maps + (long)k * M;
    const float* __restrict__ aj = maps + ((long)(1 + j) * K + k) * M;
    double num = 0.0, den = 0.0;
    for (long m = threadIdx.x; m < M; m += FD_THREADS) {
        const double c = (double)a0[m], d = (double)aj[m] - c;
        num = fma(d, d, num);
        den = fma(c, c, den);
    }
    num = at_block_sum<FD_WAVES>(num, s_num);
    den = at_block_sum<FD_WAVES>(den, s_den);
    if (threadIdx.x == 0) terms[(long)k * N + first + j] = sqrt(num / (den == 0.0 ? 1.0 : den));
}

extern "C" int scouter_map_distances_f64(const float* maps, double* terms, int first, int n, int N, int K, long M, void* stream) {
    SC_REQUIRE(maps && terms, "map_distances: null pointer (maps %p, terms %p)", (const void*)maps, (void*)terms);
    SC_REQUIRE(K > 0 && M > 0, "map_distances: bad arguments (K %d, M %ld: each must be at least 1)", K, M);
    if (int rc = fd_check_chunk("map_distances", first, n, N)) return rc;
    SC_REQUIRE(((uintptr_t)maps & 3) == 0 && ((uintptr_t)terms & 7) == 0,
               "map_distances: misaligned pointer (maps must be 4-byte, terms 8-byte aligned)");
    SC_UNSUPPORTED(K <= 65535, "map_distances: K = %d maps per sample (at most 65535)", K);
    SC_UNSUPPORTED((double)(1 + n) * K * (double)M < 2147483648.0, "map_distances: %d x %d x %ld elements are past the 32-bit "
                   "offsets", 1 + n, K, M);
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("map_distances", st, 5.0 * n * K * (double)M, 8.0 * n * K * (double)M);
    hipLaunchKernelGGL(map_distances_kernel, dim3((unsigned)n, (unsigned)K), dim3(FD_THREADS), 0, st, maps, terms, first, N, K, M);
    return sc_check_launch("map_distances");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FD_THREADS) void infidelity_finish_kernel(const double* __restrict__ dots,
                                                                       const double* __restrict__ deltas, double* __restrict__ raw,
                                                                       double* __restrict__ beta, double* __restrict__ normalized,
                                                                       long R, int N) {
    const long r = (long)blockIdx.x * FD_THREADS + threadIdx.x;
    if (r >= R) return;
    const double* __restrict__ d = dots + r * N;
    const double* __restrict__ y = deltas + r * N;
    double s_raw = 0.0, s_dd = 0.0, s_dy = 0.0;
    for (int j = 0; j < N; ++j) {
        const double gap = d[j] - y[j];
        s_raw = fma(gap, gap, s_raw);
        s_dd = fma(d[j], d[j], s_dd);
        s_dy = fma(d[j], y[j], s_dy);
    }
    const double b = s_dd == 0.0 ? 0.0 : s_dy / s_dd;
    double s_norm = 0.0;
    for (int j = 0; j < N; ++j) {
        const double gap = fma(b, d[j], -y[j]);
        s_norm = fma(gap, gap, s_norm);
    }
    raw[r] = s_raw / (double)N;
    beta[r] = b;
    normalized[r] = s_norm / (double)N;
}

extern "C" int scouter_infidelity_finish_f64(const double* dots, const double* deltas, double* raw, double* beta,
                                             double* normalized, long R, int N, void* stream) {
    SC_REQUIRE(dots && deltas && raw && beta && normalized,
               "infidelity_finish: null pointer (dots %p, deltas %p, raw %p, beta %p, normalized %p)", (const void*)dots,
               (const void*)deltas, (void*)raw, (void*)beta, (void*)normalized);
    SC_REQUIRE(R > 0 && N > 0, "infidelity_finish: bad arguments (R %ld, N %d: each must be at least 1)", R, N);
    SC_REQUIRE((((uintptr_t)dots | (uintptr_t)deltas | (uintptr_t)raw | (uintptr_t)beta | (uintptr_t)normalized) & 7) == 0,
               "infidelity_finish: misaligned pointer (every array must be 8-byte aligned)");
    SC_UNSUPPORTED(R <= 65535L * FD_THREADS, "infidelity_finish: R = %ld rows (at most %ld per call)", R, 65535L * FD_THREADS);
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("infidelity_finish", st, 12.0 * R * N, 8.0 * R * (2.0 * N + 3.0));
    hipLaunchKernelGGL(infidelity_finish_kernel, dim3((unsigned)sc_cdiv(R, FD_THREADS)), dim3(FD_THREADS), 0, st, dots, deltas, raw,
                       beta, normalized, R, N);
    return sc_check_launch("infidelity_finish");
}

__global__ __launch_bounds__(FD_THREADS) void sensitivity_finish_kernel(const double* __restrict__ terms,
                                                                        double* __restrict__ score, long R, int N) {
    const long r = (long)blockIdx.x * FD_THREADS + threadIdx.x;
    if (r >= R) return;
    const double* __restrict__ t = terms + r * N;
    double s = t[0];
    for (int j = 1; j < N; ++j) {
        const double v = t[j];
        if (s == s && !(v <= s)) s = v;                                     // a larger term, or the first NaN, which then stays
    }
    score[r] = s;
}

extern "C" int scouter_sensitivity_finish_f64(const double* terms, double* score, long R, int N, void* stream) {
    SC_REQUIRE(terms && score, "sensitivity_finish: null pointer (terms %p, score %p)", (const void*)terms, (void*)score);
    SC_REQUIRE(R > 0 && N > 0, "sensitivity_finish: bad arguments (R %ld, N %d: each must be at least 1)", R, N);
    SC_REQUIRE((((uintptr_t)terms | (uintptr_t)score) & 7) == 0,
               "sensitivity_finish: misaligned pointer (terms and score must be 8-byte aligned)");
    SC_UNSUPPORTED(R <= 65535L * FD_THREADS, "sensitivity_finish: R = %ld rows (at most %ld per call)", R, 65535L * FD_THREADS);
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("sensitivity_finish", st, (double)R * N, 8.0 * R * (N + 1.0));
    hipLaunchKernelGGL(sensitivity_finish_kernel, dim3((unsigned)sc_cdiv(R, FD_THREADS)), dim3(FD_THREADS), 0, st, terms, score, R,
                       N);
    return sc_check_launch("sensitivity_finish");
}
