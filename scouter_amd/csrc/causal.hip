// Insertion / deletion scores of a saliency map (the causal metrics of Petsiuk et al. 2018, section 4.1; the IAUC / DAUC columns
// of the SCOUTER paper): everything around the model's forwards.  For an image x [C][H][W], a class c and a map m [H][W] the
// pixels are ordered by saliency (most salient first, ties by ascending flat index, -0 = +0, NaN last), `step` of them change per
// point of a curve of n_points = ceil(HW / step) + 1 points, and point j has the min(j step, HW) first-ranked pixels changed:
//   deletion   point j = x with the changed pixels set to 0 in every channel,
//   insertion  point j = blur(x) with the changed pixels taken from x,
// p_j = exp(log_prob_j[c]) and the score is the trapezoid area (p_0 / 2 + p_1 + ... + p_{n-1} + p_n / 2) / n, n = n_points - 1.
// Every kernel has one fixed order per output element and no atomics, so two calls give the same bits.
//
// resize_bilinear_kernel: F.interpolate(mode = "bilinear", align_corners = False) of M maps, the value STORED as fp32 (cam_maps
//   of gradcam.hip recomputes it and quantises it to 256 levels, whose ties raster order would then decide): the source
//   coordinate and the blend are at_source / at_bilerp of attr_common.h, as in cam_maps.  One thread per output pixel.
// saliency_ranks_kernel: ONE workgroup of 1024 threads per map, a least-significant-digit radix sort of (key, index) pairs with
//   4-bit digits, eight passes.  key = the float's bits mapped so that an ascending unsigned order is the definition's order
//   (cz_key).  A thread owns a CONTIGUOUS run of the elements in every pass; it counts its digits into its own column of an LDS
//   table cnt[16 digits][1024 threads] (64 KiB, no atomics), the table is scanned digit-major / thread-minor, and the thread
//   then scatters its run in order from its own offsets: equal digits keep their order, the sort is stable and the result does
//   not depend on timing.  Pass 0 reads the map, passes 1 .. 6 ping-pong the pairs through two halves of a workspace, pass 7
//   writes rank[index] = position.
// separable_filter_kernel: one pass of a zero-padded klen-tap filter along rows or columns, klen fmas in tap order starting
//   from 0; the entry point runs it along rows into a caller's temporary and along columns into the output.
// causal_step_images_kernel: out[i] = point (k, mode, j) of the edit stream, decoded from g = first + i as k = g / (2 n_points),
//   mode = (g / n_points) % 2 (0 deletion, 1 insertion), j = g % n_points.  A pure select by ranks[k][p] < j step between the
//   image and zero or between the image and its blur, formed once per pixel for all C channels; W a multiple of 4 and 16-byte
//   aligned pointers: four pixels of a row per thread, 16-byte loads and stores (at_pixel_grid of attr_common.h); else one pixel
//   per thread.
// causal_curve_kernel: curve[first + i] = expf(logp[i][cols[k]]) for the same chunk.
// causal_auc_kernel: one thread per curve, the trapezoid summed in j order.
#include "attr_common.h"

constexpr int CZ_THREADS = 256;
constexpr int CZ_SORT_THREADS = 1024, CZ_SORT_WAVES = CZ_SORT_THREADS / 64;
constexpr int CZ_DIGITS = 16, CZ_PASSES = 8;
constexpr long CZ_MAX_RANKED = 1L << 20;
constexpr int CZ_MAX_KLEN = 31;

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(CZ_THREADS) void resize_bilinear_kernel(const float* __restrict__ in, float* __restrict__ out, int h,
                                                                     int w, int H, int W) {
    const long p = (long)blockIdx.x * CZ_THREADS + threadIdx.x;
    if (p >= (long)H * W) return;
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    const float* __restrict__ src = in + (long)blockIdx.y * h * w;
    int y0, y1, x0, x1;
    float ty, tx;
    at_source(y, (float)h / (float)H, h, y0, y1, ty);
    at_source(x, (float)w / (float)W, w, x0, x1, tx);
    const float* r0 = src + (long)y0 * w;
    const float* r1 = src + (long)y1 * w;
    out[(long)blockIdx.y * H * W + p] = at_bilerp(r0[x0], r0[x1], r1[x0], r1[x1], tx, ty);
}

extern "C" int scouter_resize_bilinear_f32(const float* in, float* out, int M, int h, int w, int H, int W, void* stream) {
    SC_REQUIRE(in && out, "resize_bilinear: null pointer (in %p, out %p)", (const void*)in, (void*)out);
    SC_REQUIRE(M > 0 && h > 0 && w > 0 && H > 0 && W > 0, "resize_bilinear: bad arguments (M %d, %d x %d -> %d x %d)", M, h, w, H,
               W);
    SC_REQUIRE((((uintptr_t)in | (uintptr_t)out) & 3) == 0, "resize_bilinear: misaligned pointer (in and out must be 4-byte aligned)");
    SC_UNSUPPORTED(M <= 65535, "resize_bilinear: M = %d maps (at most 65535 per call)", M);
    SC_UNSUPPORTED((long)h * w < (1L << 31) && (long)H * W < (1L << 31),
                   "resize_bilinear: map %d x %d -> %d x %d is past the 32-bit offsets", h, w, H, W);
    hipStream_t st = (hipStream_t)stream;
    const double px = (double)M * H * W;
    ScProfScope prof("resize_bilinear", st, 14.0 * px, 4.0 * (px + (double)M * h * w));
    hipLaunchKernelGGL(resize_bilinear_kernel, dim3((unsigned)sc_cdiv((long)H * W, CZ_THREADS), (unsigned)M), dim3(CZ_THREADS), 0,
                       st, in, out, h, w, H, W);
    return sc_check_launch("resize_bilinear");
}

// ---------------------------------------------------------------------------------------------------------------------------
// the sort key of a saliency value: ascending unsigned keys = most salient first.  -0 counts as +0; every NaN gets the largest
// key (less salient than every number; the stable sort orders NaNs among themselves by index)
__device__ __forceinline__ unsigned cz_key(float v) {
    unsigned u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? u : (~u & 0x7fffffffu);
}

__global__ __launch_bounds__(CZ_SORT_THREADS) void saliency_ranks_kernel(const float* __restrict__ maps, int* __restrict__ ranks,
                                                                         unsigned* ws, int n) {
    extern __shared__ __attribute__((aligned(16))) unsigned s_cnt[];      // [CZ_DIGITS][CZ_SORT_THREADS], then the wave totals
    unsigned* s_wave = s_cnt + CZ_DIGITS * CZ_SORT_THREADS;               // [CZ_SORT_WAVES]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* __restrict__ src = maps + (long)blockIdx.x * n;
    int* __restrict__ rank = ranks + (long)blockIdx.x * n;
    // the map's workspace: two halves of (keys [n], indices [n])
    unsigned* half[2] = {ws + (long)blockIdx.x * 4 * n, ws + (long)blockIdx.x * 4 * n + 2 * (long)n};
    const int per = (n + CZ_SORT_THREADS - 1) / CZ_SORT_THREADS;
    const int lo = min(tid * per, n), hi = min(lo + per, n);             // (tid * per <= 1023 * 1024)

    for (int pass = 0; pass < CZ_PASSES; ++pass) {
        const int shift = 4 * pass;
        const unsigned* in_key = half[pass & 1];                          // (pass 0 reads the map instead)
        const unsigned* in_idx = in_key + n;
        unsigned* out_key = half[(pass + 1) & 1];
        unsigned* out_idx = out_key + n;
#pragma unroll
        for (int d = 0; d < CZ_DIGITS; ++d) s_cnt[d * CZ_SORT_THREADS + tid] = 0;
        // ---- the digits of this thread's run, counted in its own column
        for (int i = lo; i < hi; ++i) {
            const unsigned key = pass == 0 ? cz_key(src[i]) : in_key[i];
            s_cnt[((key >> shift) & 15u) * CZ_SORT_THREADS + tid] += 1;
        }
        __syncthreads();
        // ---- exclusive scan of the table in (digit, thread) order: 16 consecutive entries per thread, then the workgroup
        u32x4 c[4];
        unsigned mine = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            c[q] = *(const u32x4*)(s_cnt + 16 * tid + 4 * q);
#pragma unroll
            for (int k = 0; k < 4; ++k) mine += c[q][k];
        }
        unsigned incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) s_wave[wv] = incl;
        __syncthreads();
        unsigned base = incl - mine;
        for (int k = 0; k < wv; ++k) base += s_wave[k];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            u32x4 e;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                e[k] = base;
                base += c[q][k];
            }
            *(u32x4*)(s_cnt + 16 * tid + 4 * q) = e;
        }
        __syncthreads();
        // ---- the stable scatter: the run again, in order, from this thread's own offsets
        for (int i = lo; i < hi; ++i) {
            const unsigned key = pass == 0 ? cz_key(src[i]) : in_key[i];
            const unsigned idx = pass == 0 ? (unsigned)i : in_idx[i];
            const int slot = ((key >> shift) & 15u) * CZ_SORT_THREADS + tid;
            const unsigned pos = s_cnt[slot];
            s_cnt[slot] = pos + 1;
            if (pass == CZ_PASSES - 1) {
                rank[idx] = (int)pos;
            } else {
                out_key[pos] = key;
                out_idx[pos] = idx;
            }
        }
        __syncthreads();                                                  // (the pairs are written; the table is consumed)
    }
}

extern "C" size_t scouter_saliency_ranks_workspace_bytes(int M, long HW) {
    if (M < 1 || HW < 1) return 0;
    return (size_t)M * (size_t)HW * 4 * sizeof(unsigned);
}

extern "C" int scouter_saliency_ranks_i32(const float* maps, int* ranks, int M, long HW, void* ws, size_t ws_bytes, void* stream) {
    SC_REQUIRE(M > 0 && HW > 0, "saliency_ranks: bad arguments (M %d maps of %ld elements: each must be at least 1)", M, HW);
    SC_UNSUPPORTED(HW <= CZ_MAX_RANKED, "saliency_ranks: a map of %ld elements (at most %ld)", HW, CZ_MAX_RANKED);
    SC_REQUIRE(maps && ranks && ws, "saliency_ranks: null pointer (maps %p, ranks %p, ws %p)", (const void*)maps, (void*)ranks, ws);
    SC_REQUIRE((((uintptr_t)maps | (uintptr_t)ranks | (uintptr_t)ws) & 3) == 0,
               "saliency_ranks: misaligned pointer (maps, ranks and ws must be 4-byte aligned)");
    if (ws_bytes < scouter_saliency_ranks_workspace_bytes(M, HW)) {
        sc_set_error("saliency_ranks: workspace of %zu bytes, %zu needed", ws_bytes, scouter_saliency_ranks_workspace_bytes(M, HW));
        return SC_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)(CZ_DIGITS * CZ_SORT_THREADS + CZ_SORT_WAVES) * sizeof(unsigned);
    sc_dyn_lds((const void*)saliency_ranks_kernel, lds);
    const double el = (double)M * (double)HW;
    ScProfScope prof("saliency_ranks", st, 0.0, el * (2.0 * 4.0 + 6.0 * 2.0 * 16.0 + 8.0 + 4.0));
    hipLaunchKernelGGL(saliency_ranks_kernel, dim3((unsigned)M), dim3(CZ_SORT_THREADS), lds, st, maps, ranks, (unsigned*)ws,
                       (int)HW);
    return sc_check_launch("saliency_ranks");
}

// ---------------------------------------------------------------------------------------------------------------------------
// ROWS: out[c][y][x] = sum_i taps[i] in[c][y][x + i - klen / 2]; else along y.  Zeros outside the image.
template <bool ROWS>
__global__ __launch_bounds__(CZ_THREADS) void separable_filter_kernel(const float* __restrict__ in, const float* __restrict__ taps,
                                                                      float* __restrict__ out, int H, int W, int klen) {
    __shared__ float s_w[CZ_MAX_KLEN];
    if (threadIdx.x < klen) s_w[threadIdx.x] = taps[threadIdx.x];
    __syncthreads();
    const long p = (long)blockIdx.x * CZ_THREADS + threadIdx.x;
    if (p >= (long)H * W) return;
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    const float* __restrict__ src = in + (long)blockIdx.y * H * W;
    const int r = klen / 2;
    float a = 0.f;
    for (int i = 0; i < klen; ++i) {
        const int q = (ROWS ? x : y) + i - r;
        float v = 0.f;
        if (q >= 0 && q < (ROWS ? W : H)) v = ROWS ? src[(long)y * W + q] : src[(long)q * W + x];
        a = fmaf(s_w[i], v, a);
    }
    out[(long)blockIdx.y * H * W + p] = a;
}

extern "C" int scouter_separable_filter_f32(const float* x, const float* taps, float* tmp, float* out, int C, int H, int W, int klen,
                                            void* stream) {
    SC_REQUIRE(x && taps && tmp && out, "separable_filter: null pointer (x %p, taps %p, tmp %p, out %p)", (const void*)x,
               (const void*)taps, (void*)tmp, (void*)out);
    SC_REQUIRE(C > 0 && H > 0 && W > 0, "separable_filter: bad arguments (C %d, H %d, W %d: each must be at least 1)", C, H, W);
    SC_REQUIRE(klen >= 1 && klen <= CZ_MAX_KLEN && (klen & 1), "separable_filter: klen = %d (odd, 1 <= klen <= %d)", klen,
               CZ_MAX_KLEN);
    SC_REQUIRE((((uintptr_t)x | (uintptr_t)taps | (uintptr_t)tmp | (uintptr_t)out) & 3) == 0,
               "separable_filter: misaligned pointer (x, taps, tmp and out must be 4-byte aligned)");
    SC_REQUIRE(tmp != x && tmp != out, "separable_filter: tmp must be a buffer of its own");
    SC_UNSUPPORTED(C <= 65535, "separable_filter: C = %d planes (at most 65535 per call)", C);
    SC_UNSUPPORTED((long)H * W < (1L << 31), "separable_filter: plane %d x %d is past the 32-bit offsets", H, W);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)sc_cdiv((long)H * W, CZ_THREADS), (unsigned)C);
    const double px = (double)C * H * W;
    {
        ScProfScope prof("separable_filter<rows>", st, 2.0 * klen * px, 8.0 * px);
        hipLaunchKernelGGL(separable_filter_kernel<true>, grid, dim3(CZ_THREADS), 0, st, x, taps, tmp, H, W, klen);
    }
    if (int rc = sc_check_launch("separable_filter")) return rc;
    {
        ScProfScope prof("separable_filter<cols>", st, 2.0 * klen * px, 8.0 * px);
        hipLaunchKernelGGL(separable_filter_kernel<false>, grid, dim3(CZ_THREADS), 0, st, tmp, taps, out, H, W, klen);
    }
    return sc_check_launch("separable_filter");
}

// ---------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(CZ_THREADS) void causal_step_images_kernel(const float* __restrict__ image,
                                                                        const float* __restrict__ blurred,
                                                                        const int* __restrict__ ranks, float* __restrict__ out,
                                                                        long first, int n_points, int step, int C, int H, int W) {
    const long g = first + blockIdx.x;
    const int k = (int)(g / (2L * n_points));
    const bool insertion = ((g / n_points) & 1) != 0;
    const int j = (int)(g % n_points);
    const long plane = (long)H * W;
    const long changed_below = min((long)j * step, plane);                // ranks below this have changed at point j
    const int* __restrict__ rk = ranks + (long)k * plane;
    float* __restrict__ o = out + (long)blockIdx.x * C * plane;
    constexpr int V = VEC ? 4 : 1;
    const long items = plane / V;                                         // (VEC: W, so the plane, is a multiple of 4)
    for (long i = (long)blockIdx.y * CZ_THREADS + threadIdx.x; i < items; i += (long)gridDim.y * CZ_THREADS) {
        const long p = i * V;
        bool ch[V];
        if constexpr (VEC) {
            const i32x4 r = *(const i32x4*)(rk + p);
#pragma unroll
            for (int q = 0; q < 4; ++q) ch[q] = r[q] < changed_below;
        } else {
            ch[0] = rk[p] < changed_below;
        }
        for (int c = 0; c < C; ++c) {
            if constexpr (VEC) {
                const f32x4 a = *(const f32x4*)(image + c * plane + p);
                f32x4 v;
                if (insertion) {
                    const f32x4 b = *(const f32x4*)(blurred + c * plane + p);
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = ch[q] ? a[q] : b[q];
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = ch[q] ? 0.f : a[q];
                }
                *(f32x4*)(o + c * plane + p) = v;
            } else {
                const float a = image[c * plane + p];
                o[c * plane + p] = insertion ? (ch[0] ? a : blurred[c * plane + p]) : (ch[0] ? 0.f : a);
            }
        }
    }
}

// the chunk [first, first + n) of a stream of K maps x 2 modes x n_points points
static int cz_check_chunk(const char* what, long first, int n, int K, int n_points) {
    SC_REQUIRE(n > 0 && K > 0, "%s: bad arguments (n %d, K %d: each must be at least 1)", what, n, K);
    SC_REQUIRE(n_points >= 2, "%s: n_points = %d (a curve has at least 2 points)", what, n_points);
    SC_REQUIRE(first >= 0 && first + n <= 2L * K * n_points, "%s: chunk [%ld, %ld) lies outside the stream of %d x 2 x %d images",
               what, first, first + n, K, n_points);
    return SC_OK;
}

extern "C" int scouter_causal_step_images_f32(const float* image, const float* blurred, const int* ranks, float* out, long first,
                                              int n, int K, int n_points, int step, int C, int H, int W, void* stream) {
    SC_REQUIRE(image && blurred && ranks && out, "causal_step_images: null pointer (image %p, blurred %p, ranks %p, out %p)",
               (const void*)image, (const void*)blurred, (const void*)ranks, (void*)out);
    SC_REQUIRE(C > 0 && H > 0 && W > 0, "causal_step_images: bad arguments (C %d, H %d, W %d: each must be at least 1)", C, H, W);
    if (int rc = cz_check_chunk("causal_step_images", first, n, K, n_points)) return rc;
    SC_REQUIRE(step >= 1, "causal_step_images: step = %d (at least 1)", step);
    SC_REQUIRE(((long)H * W + step - 1) / step + 1 == n_points,
               "causal_step_images: n_points = %d, but ceil(%d x %d / step %d) + 1 = %ld", n_points, H, W, step,
               ((long)H * W + step - 1) / step + 1);
    SC_REQUIRE((((uintptr_t)image | (uintptr_t)blurred | (uintptr_t)ranks | (uintptr_t)out) & 3) == 0,
               "causal_step_images: misaligned pointer (image, blurred, ranks and out must be 4-byte aligned)");
    SC_UNSUPPORTED((long)C * H * W < (1L << 31), "causal_step_images: image of %d x %d x %d elements is past the 32-bit offsets", C,
                   H, W);
    hipStream_t st = (hipStream_t)stream;
    const AtPixelGrid px =
        at_pixel_grid(H, W, CZ_THREADS, (uintptr_t)image | (uintptr_t)blurred | (uintptr_t)ranks | (uintptr_t)out);
    const double elems = (double)n * C * H * W;
    ScProfScope prof("causal_step_images", st, elems, 4.0 * (elems + 2.0 * C * (double)H * W + (double)K * H * W));
    const dim3 grid((unsigned)n, px.tiles);
    if (px.vec)
        hipLaunchKernelGGL(causal_step_images_kernel<true>, grid, dim3(CZ_THREADS), 0, st, image, blurred, ranks, out, first,
                           n_points, step, C, H, W);
    else
        hipLaunchKernelGGL(causal_step_images_kernel<false>, grid, dim3(CZ_THREADS), 0, st, image, blurred, ranks, out, first,
                           n_points, step, C, H, W);
    return sc_check_launch("causal_step_images");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CZ_THREADS) void causal_curve_kernel(const float* __restrict__ logp, const int* __restrict__ cols,
                                                                  float* __restrict__ curve, long first, int n, int n_points,
                                                                  int n_classes) {
    const int i = blockIdx.x * CZ_THREADS + threadIdx.x;
    if (i >= n) return;
    const long g = first + i;
    const int c = cols[g / (2L * n_points)];
    curve[g] = expf(logp[(long)i * n_classes + min(max(c, 0), n_classes - 1)]);      // (the host refuses an index outside)
}

extern "C" int scouter_causal_curve_f32(const float* logp, const int* cols, float* curve_flat, long first, int n, int K,
                                        int n_points, int n_classes, void* stream) {
    SC_REQUIRE(logp && cols && curve_flat, "causal_curve: null pointer (logp %p, cols %p, curve_flat %p)", (const void*)logp,
               (const void*)cols, (void*)curve_flat);
    if (int rc = cz_check_chunk("causal_curve", first, n, K, n_points)) return rc;
    SC_REQUIRE(n_classes > 0, "causal_curve: n_classes = %d (at least 1)", n_classes);
    SC_REQUIRE((((uintptr_t)logp | (uintptr_t)cols | (uintptr_t)curve_flat) & 3) == 0,
               "causal_curve: misaligned pointer (logp, cols and curve_flat must be 4-byte aligned)");
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("causal_curve", st, 8.0 * n, 12.0 * n);
    hipLaunchKernelGGL(causal_curve_kernel, dim3((unsigned)sc_cdiv(n, CZ_THREADS)), dim3(CZ_THREADS), 0, st, logp, cols, curve_flat,
                       first, n, n_points, n_classes);
    return sc_check_launch("causal_curve");
}

__global__ __launch_bounds__(CZ_THREADS) void causal_auc_kernel(const float* __restrict__ curves, float* __restrict__ scores, long R,
                                                                int n_points) {
    const long r = (long)blockIdx.x * CZ_THREADS + threadIdx.x;
    if (r >= R) return;
    const float* __restrict__ p = curves + r * n_points;
    const int n_steps = n_points - 1;
    float a = 0.5f * p[0];
    for (int j = 1; j < n_steps; ++j) a += p[j];
    a += 0.5f * p[n_steps];
    scores[r] = a / (float)n_steps;
}

extern "C" int scouter_causal_auc_f32(const float* curves, float* scores, long R, int n_points, void* stream) {
    SC_REQUIRE(curves && scores, "causal_auc: null pointer (curves %p, scores %p)", (const void*)curves, (void*)scores);
    SC_REQUIRE(R > 0, "causal_auc: R = %ld curves (at least 1)", R);
    SC_REQUIRE(n_points >= 2, "causal_auc: n_points = %d (a curve has at least 2 points)", n_points);
    SC_REQUIRE((((uintptr_t)curves | (uintptr_t)scores) & 3) == 0,
               "causal_auc: misaligned pointer (curves and scores must be 4-byte aligned)");
    SC_UNSUPPORTED(R <= 65535L * CZ_THREADS, "causal_auc: R = %ld curves (at most %ld per call)", R, 65535L * CZ_THREADS);
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("causal_auc", st, (double)R * n_points, 4.0 * R * (n_points + 1.0));
    hipLaunchKernelGGL(causal_auc_kernel, dim3((unsigned)sc_cdiv(R, CZ_THREADS)), dim3(CZ_THREADS), 0, st, curves, scores, R,
                       n_points);
    return sc_check_launch("causal_auc");
}
