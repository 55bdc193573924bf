// LIME (Ribeiro et al. 2016) and KernelSHAP (Lundberg & Lee 2017): a linear surrogate over d <= 128 superpixels, fitted to the
// class probabilities of N perturbed copies of an image.  Six kernels, each with one fixed summation order per output element and
// no atomics, so two calls give the same bits (include/scouter_hip.h has the definitions).
//
// slic_update_kernel: one workgroup per (segment, image).  It scans the 3 x 3 grid cells around the segment's own cell (or the
//   whole image: window = 0), once per quantity -- the count, y, x and the C colours -- each a float64 sum in thread order, lanes
//   by butterfly, waves in order (at_block_sum), rounded once to fp32.  An empty segment keeps its centre; its mean colour is 0.
// slic_assign_kernel: one thread per pixel, the image's d centres in LDS; the 3 x 3 cells around the pixel's home cell in
//   ascending label order, a strictly smaller D^2 wins, so a tie goes to the smallest label.
// segment_images_kernel: out[n][c][p] = z[n][labels[p]] ? image[c][p] : hide -- a select, every value an exact copy.  A workgroup
//   belongs to ONE sample row (blockIdx.x), its d bytes (and the d x C mean colours) in LDS; 16-byte accesses when W allows.
// surrogate_accumulate_kernel: one thread per entry of S [d + 1][d + 1] and T [d + 1][K], which STARTS from the stored value and
//   adds the rows of a chunk in ascending n: chunks of any length give the bits of one call.  Rows are staged SG_NP at a time.
// surrogate_solve_kernel: one workgroup per image: the reduced normal equations G | R written into a float64 workspace, a
//   right-looking Cholesky factorisation in place, then one thread per class runs the two triangular solves.
// segment_paint_kernel: out[b][k][p] = (float) coef[b][k][labels[b][p]], the coefficient row in LDS.
// Every label a kernel indexes with is clamped to [0, d - 1], so no value moves an address.
#include "attr_common.h"

constexpr int SG_MAX_D = 128;                  // segments per image
constexpr int SG_MAX_C = 30;                   // image channels (the centres of an image fit 16 KiB of LDS)
constexpr int SG_THREADS = 256, SG_WAVES = SG_THREADS / 64;
constexpr int SG_NP = 32;                      // sample rows staged in LDS at a time
constexpr int SG_MODE_LIME = 0, SG_MODE_SHAP = 1;

typedef int sg_i32x4 __attribute__((ext_vector_type(4)));

// the first pixel of cell i of an axis of `size` pixels cut into g cells (pixel y lies in cell y g / size): ceil(i size / g)
__host__ __device__ __forceinline__ int sg_cell_start(int i, int size, int g) { return (int)(((long)i * size + g - 1) / g); }

__device__ __forceinline__ int sg_clamp(int l, int d) { return min(max(l, 0), d - 1); }

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SG_THREADS) void slic_update_kernel(const float* __restrict__ images, const int* __restrict__ labels,
                                                                 float* __restrict__ centres, float* __restrict__ means, int C,
                                                                 int H, int W, int gy, int gx, int window) {
    __shared__ double s_part[2][SG_WAVES];
    const int seg = blockIdx.x, b = blockIdx.y, d = gy * gx, tid = threadIdx.x;
    int y0 = 0, y1 = H, x0 = 0, x1 = W;
    if (window) {
        const int i = seg / gx, j = seg - i * gx;
        y0 = sg_cell_start(max(i - 1, 0), H, gy); y1 = sg_cell_start(min(i + 2, gy), H, gy);
        x0 = sg_cell_start(max(j - 1, 0), W, gx); x1 = sg_cell_start(min(j + 2, gx), W, gx);
    }
    const int ww = x1 - x0;
    const long items = (long)(y1 - y0) * ww, plane = (long)H * W;
    const int* __restrict__ lab = labels + (long)b * plane;
    const float* __restrict__ img = images + (long)b * C * plane;
    float* __restrict__ ctr = centres + ((long)b * d + seg) * (C + 2);
    float* __restrict__ mean = means + ((long)b * d + seg) * C;
    double count = 0.0;                                         // (thread 0)
    for (int q = 0; q < C + 3; ++q) {                           // the count, y, x, then the C colours
        double a = 0.0;
        for (long t = tid; t < items; t += SG_THREADS) {
            const int ty = (int)(t / ww), y = y0 + ty, x = x0 + (int)(t - (long)ty * ww);
            const long p = (long)y * W + x;
            if (lab[p] == seg) a += q == 0 ? 1.0 : q == 1 ? (double)y : q == 2 ? (double)x : (double)img[(q - 3) * plane + p];
        }
        const double tot = at_block_sum<SG_WAVES>(a, s_part[q & 1]);      // (two buffers: the sum after next reuses this one)
        if (tid == 0) {
            if (q == 0) count = tot;
            else if (count > 0.0) {
                const float v = (float)(tot / count);
                if (q == 1) ctr[C] = v;
                else if (q == 2) ctr[C + 1] = v;
                else { ctr[q - 3] = v; mean[q - 3] = v; }
            } else if (q >= 3) {
                mean[q - 3] = 0.f;
            }
        }
    }
}

static int sg_check_image(const char* what, int B, int C, int H, int W) {
    SC_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "%s: bad arguments (B %d, C %d, H %d, W %d: each must be at least 1)", what, B, C,
               H, W);
    SC_UNSUPPORTED(C <= SG_MAX_C, "%s: C = %d channels (at most %d)", what, C, SG_MAX_C);
    SC_UNSUPPORTED((long)C * H * W < (1L << 31), "%s: image of %d x %d x %d elements is past the 32-bit offsets", what, C, H, W);
    SC_UNSUPPORTED(B <= 65535, "%s: B = %d (at most 65535)", what, B);
    return SC_OK;
}

static int sg_check_d(const char* what, int d) {
    SC_REQUIRE(d >= 1 && d <= SG_MAX_D, "%s: d = %d segments (1 <= d <= %d)", what, d, SG_MAX_D);
    return SC_OK;
}

static int sg_check_grid(const char* what, int H, int W, int gy, int gx, bool inside) {
    SC_REQUIRE(gy >= 1 && gx >= 1 && gy <= SG_MAX_D && gx <= SG_MAX_D, "%s: grid %d x %d (each at least 1)", what, gy, gx);
    if (int rc = sg_check_d(what, gy * gx)) return rc;
    SC_REQUIRE(!inside || (gy <= H && gx <= W), "%s: grid %d x %d is larger than the image %d x %d", what, gy, gx, H, W);
    return SC_OK;
}

extern "C" int scouter_slic_update_f32(const float* images, const int* labels, float* centres, float* means, int B, int C, int H,
                                       int W, int gy, int gx, int window, void* stream) {
    SC_REQUIRE(images && labels && centres && means, "slic_update: null pointer (images %p, labels %p, centres %p, means %p)",
               (const void*)images, (const void*)labels, (void*)centres, (void*)means);
    SC_REQUIRE((((uintptr_t)images | (uintptr_t)labels | (uintptr_t)centres | (uintptr_t)means) & 3) == 0,
               "slic_update: misaligned pointer (all four must be 4-byte aligned)");
    if (int rc = sg_check_image("slic_update", B, C, H, W)) return rc;
    if (int rc = sg_check_grid("slic_update", H, W, gy, gx, window != 0)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const double scanned = (double)B * gy * gx * (window ? 9.0 * H * W / (gy * gx) : (double)H * W);
    ScProfScope prof("slic_update", st, scanned * (C + 3), 4.0 * scanned * (C + 3));
    hipLaunchKernelGGL(slic_update_kernel, dim3((unsigned)(gy * gx), (unsigned)B), dim3(SG_THREADS), 0, st, images, labels, centres,
                       means, C, H, W, gy, gx, window);
    return sc_check_launch("slic_update");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SG_THREADS) void slic_assign_kernel(const float* __restrict__ images, const float* __restrict__ centres,
                                                                 int* __restrict__ labels, int C, int H, int W, int gy, int gx,
                                                                 float lambda) {
    __shared__ float s_c[SG_MAX_D * (SG_MAX_C + 2)];
    const int b = blockIdx.y, d = gy * gx, stride = C + 2, tid = threadIdx.x;
    for (int i = tid; i < d * stride; i += SG_THREADS) s_c[i] = centres[(long)b * d * stride + i];
    __syncthreads();
    const long plane = (long)H * W;
    const float* __restrict__ img = images + (long)b * C * plane;
    for (long p = (long)blockIdx.x * SG_THREADS + tid; p < plane; p += (long)gridDim.x * SG_THREADS) {
        const int y = (int)(p / W), x = (int)(p - (long)y * W);
        const int ci = min((int)((long)y * gy / H), gy - 1), cj = min((int)((long)x * gx / W), gx - 1);
        float best = INFINITY;
        int bl = ci * gx + cj;                                   // (every distance a NaN: the home cell)
        for (int i = max(ci - 1, 0); i <= min(ci + 1, gy - 1); ++i) {
            for (int j = max(cj - 1, 0); j <= min(cj + 1, gx - 1); ++j) {      // (ascending label)
                const int l = i * gx + j;
                const float* __restrict__ c = s_c + l * stride;
                float dc = 0.f;
                for (int ch = 0; ch < C; ++ch) {
                    const float df = img[ch * plane + p] - c[ch];
                    dc = fmaf(df, df, dc);
                }
                const float dy = (float)y - c[C], dx = (float)x - c[C + 1];
                const float D = fmaf(lambda, fmaf(dy, dy, dx * dx), dc);
                if (D < best) { best = D; bl = l; }
            }
        }
        labels[(long)b * plane + p] = bl;
    }
}

extern "C" int scouter_slic_assign_f32(const float* images, const float* centres, int* labels, int B, int C, int H, int W, int gy,
                                       int gx, float lambda, void* stream) {
    SC_REQUIRE(images && centres && labels, "slic_assign: null pointer (images %p, centres %p, labels %p)", (const void*)images,
               (const void*)centres, (void*)labels);
    SC_REQUIRE((((uintptr_t)images | (uintptr_t)centres | (uintptr_t)labels) & 3) == 0,
               "slic_assign: misaligned pointer (all three must be 4-byte aligned)");
    if (int rc = sg_check_image("slic_assign", B, C, H, W)) return rc;
    if (int rc = sg_check_grid("slic_assign", H, W, gy, gx, true)) return rc;
    SC_REQUIRE(lambda == lambda, "slic_assign: lambda is not a number");
    hipStream_t st = (hipStream_t)stream;
    const double px = (double)B * H * W;
    ScProfScope prof("slic_assign", st, px * 9.0 * (3.0 * C + 6.0), 4.0 * px * (C + 1));
    const long tiles = ((long)H * W + SG_THREADS - 1) / SG_THREADS;
    hipLaunchKernelGGL(slic_assign_kernel, dim3((unsigned)(tiles > 65535 ? 65535 : tiles), (unsigned)B), dim3(SG_THREADS), 0, st,
                       images, centres, labels, C, H, W, gy, gx, lambda);
    return sc_check_launch("slic_assign");
}

// ---------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(SG_THREADS) void segment_images_kernel(const float* __restrict__ image, const int* __restrict__ labels,
                                                                    const unsigned char* __restrict__ z,
                                                                    const float* __restrict__ means, float fill,
                                                                    float* __restrict__ out, int d, int C, int H, int W) {
    __shared__ unsigned char s_z[SG_MAX_D];
    __shared__ float s_m[SG_MAX_D * SG_MAX_C];
    const int n = blockIdx.x, tid = threadIdx.x;
    if (tid < d) s_z[tid] = z[(long)n * d + tid];
    if (means)
        for (int i = tid; i < d * C; i += SG_THREADS) s_m[i] = means[i];
    __syncthreads();
    const long plane = (long)H * W;
    float* __restrict__ o = out + (long)n * C * plane;
    constexpr int V = VEC ? 4 : 1;
    const int wq = W / V;                                       // (VEC: W is a multiple of 4)
    const long items = (long)H * wq;
    for (long i = (long)blockIdx.y * SG_THREADS + tid; i < items; i += (long)gridDim.y * SG_THREADS) {
        const long p = i * V;                                    // (rows are whole groups of V: flat index = V i)
        int l[V];
        if constexpr (VEC) {
            const sg_i32x4 t = *(const sg_i32x4*)(labels + p);
#pragma unroll
            for (int k = 0; k < 4; ++k) l[k] = sg_clamp(t[k], d);
        } else {
            l[0] = sg_clamp(labels[p], d);
        }
        bool keep[V];
#pragma unroll
        for (int k = 0; k < V; ++k) keep[k] = s_z[l[k]] != 0;
        for (int c = 0; c < C; ++c) {
            float v[V];
            at_load<V>(image + c * plane + p, v);
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = keep[k] ? v[k] : (means ? s_m[l[k] * C + c] : fill);
            if constexpr (VEC) *(f32x4*)(o + c * plane + p) = f32x4{v[0], v[1], v[2], v[3]};
            else o[c * plane + p] = v[0];
        }
    }
}

extern "C" int scouter_segment_images_f32(const float* image, const int* labels, const unsigned char* z, const float* means,
                                          float fill, float* out, int N, int d, int C, int H, int W, void* stream) {
    SC_REQUIRE(image && labels && z && out, "segment_images: null pointer (image %p, labels %p, z %p, out %p)", (const void*)image,
               (const void*)labels, (const void*)z, (void*)out);
    SC_REQUIRE((((uintptr_t)image | (uintptr_t)labels | (uintptr_t)means | (uintptr_t)out) & 3) == 0,
               "segment_images: misaligned pointer (image, labels, means and out must be 4-byte aligned)");
    SC_REQUIRE(N > 0, "segment_images: bad arguments (N %d: at least 1)", N);
    if (int rc = sg_check_image("segment_images", 1, C, H, W)) return rc;
    if (int rc = sg_check_d("segment_images", d)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const AtPixelGrid px = at_pixel_grid(H, W, SG_THREADS, (uintptr_t)image | (uintptr_t)labels | (uintptr_t)out);
    const double elems = (double)N * C * H * W;
    ScProfScope prof("segment_images", st, elems, 4.0 * (2.0 * elems + (double)N * H * W));
    const dim3 grid((unsigned)N, px.tiles);
    if (px.vec)
        hipLaunchKernelGGL(segment_images_kernel<true>, grid, dim3(SG_THREADS), 0, st, image, labels, z, means, fill, out, d, C, H, W);
    else
        hipLaunchKernelGGL(segment_images_kernel<false>, grid, dim3(SG_THREADS), 0, st, image, labels, z, means, fill, out, d, C, H,
                           W);
    return sc_check_launch("segment_images");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SG_THREADS) void surrogate_accumulate_kernel(const float* __restrict__ logp, const int* __restrict__ cols,
                                                                          const unsigned char* __restrict__ z, double* __restrict__ S,
                                                                          double* __restrict__ T, double* __restrict__ yref,
                                                                          long first, int N, int n_classes, int K, int d, int mode,
                                                                          double kernel_width) {
    __shared__ unsigned char s_z[SG_NP][SG_MAX_D + 1];          // z^ = (1, z)
    __shared__ double s_pi[SG_NP];
    const int tid = threadIdx.x, D1 = d + 1;
    const long nS = (long)D1 * D1, total = nS + (long)D1 * K;
    const long e = (long)blockIdx.x * SG_THREADS + tid;
    const bool live = e < total, isS = e < nS;
    int a = 0, c = 0, col = 0;
    if (live) {
        if (isS) { a = (int)(e / D1); c = (int)(e - (long)a * D1); }
        else { a = (int)((e - nS) / K); c = (int)((e - nS) - (long)a * K); col = min(max(cols[c], 0), n_classes - 1); }
    }
    double* __restrict__ dst = isS ? S + e : T + (e - nS);
    double acc = live ? *dst : 0.0;
    const double kw2 = kernel_width * kernel_width;

    for (int n0 = 0; n0 < N; n0 += SG_NP) {
        const int np = min(SG_NP, N - n0);
        __syncthreads();                                         // (the previous piece is consumed)
        for (int i = tid; i < np * D1; i += SG_THREADS) {
            const int j = i / D1, f = i - j * D1;
            s_z[j][f] = f == 0 ? 1 : (z[(long)(n0 + j) * d + f - 1] != 0);
        }
        __syncthreads();
        if (tid < np) {
            double pi = 1.0;
            if (mode == SG_MODE_LIME) {
                int cnt = 0;
                for (int f = 1; f <= d; ++f) cnt += s_z[tid][f];
                const double dist = cnt == 0 ? 1.0 : 1.0 - sqrt((double)cnt / (double)d);
                pi = sqrt(exp(-(dist * dist) / kw2));
            }
            s_pi[tid] = pi;
        }
        __syncthreads();
        if (live) {
            for (int j = 0; j < np; ++j) {
                if (isS) {
                    if (s_z[j][a] & s_z[j][c]) acc += s_pi[j];
                } else if (s_z[j][a]) {
                    acc += s_pi[j] * exp((double)logp[(long)(n0 + j) * n_classes + col]);
                }
            }
        }
    }
    if (live) *dst = acc;

    // the targets of the full row (0) and the empty row (1) of the whole sample matrix, when this chunk holds them
    if (blockIdx.x == 0 && yref) {
        for (int k = tid; k < K; k += SG_THREADS) {
            const int ck = min(max(cols[k], 0), n_classes - 1);
            for (int r = 0; r < 2; ++r) {
                const long n = r - first;
                if (n >= 0 && n < N) yref[r * K + k] = exp((double)logp[n * n_classes + ck]);
            }
        }
    }
}

extern "C" int scouter_surrogate_accumulate_f64(const float* logp, const int* cols, const unsigned char* z, double* S, double* T,
                                                double* yref, long first, int N, int n_classes, int K, int d, int mode,
                                                double kernel_width, void* stream) {
    SC_REQUIRE(logp && cols && z && S && T, "surrogate_accumulate: null pointer (logp %p, cols %p, z %p, S %p, T %p)",
               (const void*)logp, (const void*)cols, (const void*)z, (void*)S, (void*)T);
    SC_REQUIRE((((uintptr_t)logp | (uintptr_t)cols) & 3) == 0 && (((uintptr_t)S | (uintptr_t)T | (uintptr_t)yref) & 7) == 0,
               "surrogate_accumulate: misaligned pointer (logp, cols: 4 bytes; S, T, yref: 8 bytes)");
    SC_REQUIRE(N > 0 && n_classes > 0 && first >= 0,
               "surrogate_accumulate: bad arguments (N %d, n_classes %d: each at least 1; first %ld: at least 0)", N, n_classes, first);
    SC_REQUIRE(K > 0, "surrogate_accumulate: K = %d classes (at least 1)", K);
    if (int rc = sg_check_d("surrogate_accumulate", d)) return rc;
    SC_REQUIRE(mode == SG_MODE_LIME || mode == SG_MODE_SHAP, "surrogate_accumulate: mode %d (0: LIME weights, 1: unit weights)", mode);
    SC_REQUIRE(mode != SG_MODE_LIME || kernel_width > 0.0, "surrogate_accumulate: kernel_width %g must be positive", kernel_width);
    const long total = (long)(d + 1) * (d + 1) + (long)(d + 1) * K;
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("surrogate_accumulate", st, 2.0 * N * (double)total, 16.0 * total + 4.0 * N * (double)n_classes + (double)N * d);
    hipLaunchKernelGGL(surrogate_accumulate_kernel, dim3((unsigned)sc_cdiv(total, SG_THREADS)), dim3(SG_THREADS), 0, st, logp, cols, z,
                       S, T, yref, first, N, n_classes, K, d, mode, kernel_width);
    return sc_check_launch("surrogate_accumulate");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SG_THREADS) void surrogate_solve_kernel(const double* __restrict__ S, const double* __restrict__ T,
                                                                     const double* __restrict__ yref, double* __restrict__ ws,
                                                                     double* __restrict__ coef, double* __restrict__ icpt, int d,
                                                                     int K, int mode, double alpha) {
    __shared__ double s_piv;
    const int b = blockIdx.x, tid = threadIdx.x, D1 = d + 1;
    const bool shap = mode == SG_MODE_SHAP;
    const int m = shap ? d - 1 : d, ld = m + K, e = d - 1;      // (e: the feature KernelSHAP eliminates)
    const double* __restrict__ Sb = S + (long)b * D1 * D1;
    const double* __restrict__ Tb = T + (long)b * D1 * K;
    const double* __restrict__ yF = shap ? yref + (long)b * 2 * K : nullptr;
    const double* __restrict__ yE = shap ? yF + K : nullptr;
    double* G = ws + (long)b * d * (d + K);                       // [m][m + K]: G | R, row stride ld
    auto S2 = [&](int r, int c) { return Sb[(long)(r + 1) * D1 + c + 1]; };
    auto S1 = [&](int r) { return Sb[(long)(r + 1) * D1]; };
    auto T1 = [&](int r, int k) { return Tb[(long)(r + 1) * K + k]; };
    const double S00 = Sb[0];

    for (int i = tid; i < m * ld; i += SG_THREADS) {
        const int r = i / ld, c = i - r * ld;
        double v;
        if (c < m) {
            v = shap ? S2(r, c) - S2(r, e) - S2(e, c) + S2(e, e) : S2(r, c) - S1(r) * S1(c) / S00;
            if (r == c) v += alpha;
        } else {
            const int k = c - m;
            v = shap ? T1(r, k) - T1(e, k) - yE[k] * (S1(r) - S1(e)) - (yF[k] - yE[k]) * (S2(r, e) - S2(e, e))
                     : T1(r, k) - S1(r) * Tb[k] / S00;
        }
        G[i] = v;
    }
    bool bad = !shap && !(S00 > 0.0);

    // ---- G = L L^T in place (the lower triangle), column by column
    for (int j = 0; j < m && !bad; ++j) {
        __syncthreads();
        if (tid == 0) s_piv = G[(long)j * ld + j];
        __syncthreads();
        const double piv = s_piv;
        if (!(piv > 0.0)) { bad = true; break; }                  // (the same value in every thread)
        const double l = sqrt(piv);
        for (int i = j + 1 + tid; i < m; i += SG_THREADS) G[(long)i * ld + j] /= l;
        if (tid == 0) G[(long)j * ld + j] = l;
        __syncthreads();
        const int r = m - j - 1;
        for (int t = tid; t < r * r; t += SG_THREADS) {
            const int ii = j + 1 + t / r, cc = j + 1 + t % r;
            if (cc <= ii) G[(long)ii * ld + cc] -= G[(long)ii * ld + j] * G[(long)cc * ld + j];
        }
    }
    __syncthreads();

    // ---- one thread per class: L y = R, L^T w = y, then the outputs
    const double nan = __builtin_nan("");
    for (int k = tid; k < K; k += SG_THREADS) {
        double* __restrict__ w = coef + ((long)b * K + k) * d;
        if (bad) {
            for (int a = 0; a < d; ++a) w[a] = nan;
            icpt[(long)b * K + k] = shap ? yE[k] : nan;
            continue;
        }
        double* R = G + m + k;                                   // R[i ld]
        for (int i = 0; i < m; ++i) {
            double v = R[(long)i * ld];
            for (int c = 0; c < i; ++c) v -= G[(long)i * ld + c] * R[(long)c * ld];
            R[(long)i * ld] = v / G[(long)i * ld + i];
        }
        for (int i = m - 1; i >= 0; --i) {
            double v = R[(long)i * ld];
            for (int c = i + 1; c < m; ++c) v -= G[(long)c * ld + i] * R[(long)c * ld];
            R[(long)i * ld] = v / G[(long)i * ld + i];
        }
        double sum = 0.0;
        for (int a = 0; a < m; ++a) {
            const double v = R[(long)a * ld];
            w[a] = v;
            sum += shap ? v : S1(a) * v;
        }
        if (shap) {
            w[e] = (yF[k] - yE[k]) - sum;
            icpt[(long)b * K + k] = yE[k];
        } else {
            icpt[(long)b * K + k] = (Tb[k] - sum) / S00;
        }
    }
}

extern "C" size_t scouter_surrogate_solve_workspace_bytes(int B, int d, int K) {
    if (B < 1 || d < 1 || K < 1) return 0;
    return (size_t)B * d * ((size_t)d + K) * sizeof(double);
}

extern "C" int scouter_surrogate_solve_f64(const double* S, const double* T, const double* yref, double* coef, double* icpt, int B,
                                           int d, int K, int mode, double alpha, void* ws, size_t ws_bytes, void* stream) {
    SC_REQUIRE(S && T && coef && icpt && ws, "surrogate_solve: null pointer (S %p, T %p, coef %p, icpt %p, ws %p)", (const void*)S,
               (const void*)T, (void*)coef, (void*)icpt, ws);
    SC_REQUIRE(mode == SG_MODE_LIME || mode == SG_MODE_SHAP, "surrogate_solve: mode %d (0: LIME, 1: KernelSHAP)", mode);
    SC_REQUIRE(mode != SG_MODE_SHAP || yref, "surrogate_solve: null pointer (yref, which KernelSHAP needs)");
    SC_REQUIRE((((uintptr_t)S | (uintptr_t)T | (uintptr_t)yref | (uintptr_t)coef | (uintptr_t)icpt | (uintptr_t)ws) & 7) == 0,
               "surrogate_solve: misaligned pointer (all must be 8-byte aligned)");
    SC_REQUIRE(B > 0, "surrogate_solve: bad arguments (B %d: at least 1)", B);
    SC_REQUIRE(K > 0, "surrogate_solve: K = %d classes (at least 1)", K);
    if (int rc = sg_check_d("surrogate_solve", d)) return rc;
    SC_REQUIRE(alpha == alpha && alpha >= 0.0, "surrogate_solve: ridge alpha %g must be a number and at least 0", alpha);
    SC_UNSUPPORTED(B <= 65535 && K <= (1 << 20), "surrogate_solve: B = %d, K = %d (at most 65535 and 2^20)", B, K);
    if (ws_bytes < scouter_surrogate_solve_workspace_bytes(B, d, K)) {
        sc_set_error("surrogate_solve: workspace of %zu bytes, %zu needed", ws_bytes, scouter_surrogate_solve_workspace_bytes(B, d, K));
        return SC_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("surrogate_solve", st, (double)B * ((double)d * d * d / 3.0 + 2.0 * d * d * (double)K),
                     8.0 * B * (2.0 * (d + 1.0) * (d + 1.0 + K)));
    hipLaunchKernelGGL(surrogate_solve_kernel, dim3((unsigned)B), dim3(SG_THREADS), 0, st, S, T, yref, (double*)ws, coef, icpt, d, K,
                       mode, alpha);
    return sc_check_launch("surrogate_solve");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SG_THREADS) void segment_paint_kernel(const double* __restrict__ coef, const int* __restrict__ labels,
                                                                   float* __restrict__ out, int K, int d, long plane) {
    __shared__ float s_w[SG_MAX_D];
    const int bk = blockIdx.y, b = bk / K, tid = threadIdx.x;
    if (tid < d) s_w[tid] = (float)coef[(long)bk * d + tid];
    __syncthreads();
    const int* __restrict__ lab = labels + (long)b * plane;
    float* __restrict__ o = out + (long)bk * plane;
    for (long p = (long)blockIdx.x * SG_THREADS + tid; p < plane; p += (long)gridDim.x * SG_THREADS) o[p] = s_w[sg_clamp(lab[p], d)];
}

extern "C" int scouter_segment_paint_f32(const double* coef, const int* labels, float* out, int B, int K, int d, int H, int W,
                                         void* stream) {
    SC_REQUIRE(coef && labels && out, "segment_paint: null pointer (coef %p, labels %p, out %p)", (const void*)coef,
               (const void*)labels, (void*)out);
    SC_REQUIRE(((uintptr_t)coef & 7) == 0 && (((uintptr_t)labels | (uintptr_t)out) & 3) == 0,
               "segment_paint: misaligned pointer (coef: 8 bytes; labels, out: 4 bytes)");
    SC_REQUIRE(B > 0 && H > 0 && W > 0, "segment_paint: bad arguments (B %d, H %d, W %d: each must be at least 1)", B, H, W);
    SC_REQUIRE(K > 0, "segment_paint: K = %d classes (at least 1)", K);
    if (int rc = sg_check_d("segment_paint", d)) return rc;
    SC_UNSUPPORTED((long)H * W < (1L << 31), "segment_paint: map %d x %d is past the 32-bit offsets", H, W);
    SC_UNSUPPORTED((long)B * K <= 65535, "segment_paint: B K = %ld maps (at most 65535)", (long)B * K);
    hipStream_t st = (hipStream_t)stream;
    const double px = (double)B * K * H * W;
    ScProfScope prof("segment_paint", st, px, 8.0 * px);
    const long tiles = ((long)H * W + SG_THREADS - 1) / SG_THREADS;
    hipLaunchKernelGGL(segment_paint_kernel, dim3((unsigned)(tiles > 4096 ? 4096 : tiles), (unsigned)(B * K)), dim3(SG_THREADS), 0,
                       st, coef, labels, out, K, d, (long)H * W);
    return sc_check_launch("segment_paint");
}
